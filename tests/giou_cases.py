"""The inputs of the GIoU op tests, shared by test_gpu_giou.py (which runs them through the kernels) and test_giou_ref.py (which
shows on the same inputs that each seeded mistake of giou_ref.py moves the results by far more than the GPU bounds, and that the
separation condition below holds).

Layouts are those of focal_cases.py.  Logits and labels come from loss_ref.palette_batch / continuous_batch; the offsets of every
positive anchor are then redrawn (ground truth N(0, 1.5), prediction around it, a third of them with the centre pushed far away:
disjoint boxes), and a GEOMETRY PALETTE is written onto the first positives of every sample:
  identical boxes; touching boxes (t2 = t3 = 0 on both sides, centres from {0, +-5, +-10, +-20}: cx = 0, +-1/2, +-1, +-2 and unit
  sizes are exact in fp32 under division and under multiplication by a reciprocal, so every tie is an exact tie on the GPU too);
  disjoint in x only, and in both axes; prediction strictly inside the ground truth, and the reverse; offsets beyond +-100 in
  each component, +-1e30 included; t2 = 100 against g2 = 0, and t2 = -100.
Every positive outside the palette's tie entries is SEPARATED (giou_ref.separated): each pair of coordinates the definition
compares differs by more than 1e-5 * max(|a|, |b|, 1), so the fp32 branch decisions are the float64 ones; a draw that is not is
drawn again here, and test_giou_ref.py asserts the condition on what comes out."""
import zlib

import numpy as np

import focal_cases as fc
import giou_ref as gr
import loss_ref as lr

VGG300, BIG32, TINY, A1024, A1025, MID = fc.VGG300, fc.BIG32, fc.TINY, fc.A1024, fc.A1025, fc.MID

# (predicted offsets, label offsets, holds an exact tie)
PALETTE = [
    ((1.5, -2.25, 3.0, -4.0), (1.5, -2.25, 3.0, -4.0), True),          # identical
    ((0.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 0.0), True),                # identical unit boxes
    ((10.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 0.0), True),               # touching in x (x0p == x1g), identical in y
    ((-10.0, 10.0, 0.0, 0.0), (0.0, 0.0, 0.0, 0.0), True),             # touching in both (a corner)
    ((5.0, -5.0, 0.0, 0.0), (0.0, 0.0, 0.0, 0.0), False),              # half overlapping unit boxes: no pair coincides
    ((20.0, 5.0, 0.0, 0.0), (10.0, 0.0, 0.0, 0.0), True),              # touching in x, half overlapping in y
    ((5.0, 0.0, 0.0, 0.0), (-5.0, 0.0, 0.0, 0.0), True),               # touching in x at 0, identical in y
    ((0.0, 20.0, 0.0, 0.0), (0.0, -20.0, 0.0, 0.0), True),             # identical in x, far apart in y
    ((30.0, 1.0, 0.5, 0.25), (0.0, 0.25, -0.25, 0.125), False),        # disjoint in x only
    ((30.0, -40.0, 0.5, 0.25), (0.0, 0.25, -0.25, 0.125), False),      # disjoint in both axes
    ((-35.0, 45.0, -1.0, 0.75), (2.0, -1.0, 0.5, -0.5), False),        # disjoint in both axes, the other quadrant
    ((0.5, -0.25, -5.0, -6.0), (0.0, 0.0, 2.0, 3.0), False),           # prediction strictly inside the ground truth
    ((0.25, 0.5, 4.0, 3.5), (-0.5, 0.25, -3.0, -2.0), False),          # ground truth strictly inside the prediction
    ((150.0, 0.25, 0.5, -0.5), (1.0, -1.0, 0.25, 0.5), False),         # t0 beyond the clamp
    ((0.25, -101.0, 0.5, -0.5), (1.0, -1.0, 0.25, 0.5), False),        # t1
    ((0.25, 0.5, 120.0, -0.5), (1.0, -1.0, 0.25, 0.5), False),         # t2
    ((0.25, 0.5, 0.75, -250.0), (1.0, -1.0, 0.25, 0.5), False),        # t3
    ((100.5, 0.25, 0.5, -0.5), (95.0, -1.0, 0.25, 0.5), False),        # t0 just beyond, the boxes overlapping: the clamp cuts a
    ((0.25, -100.25, 0.5, -0.5), (1.0, -99.0, 0.25, 0.5), False),      # ... gradient that would not be small; t1,
    ((0.25, 0.5, 101.0, -0.5), (1.0, -1.0, 99.0, 0.5), False),         # ... t2 (widths exp(20) and exp(19.8)),
    ((0.25, 0.5, 0.75, -102.0), (1.0, -1.0, 0.25, -99.5), False),      # ... t3
    ((1e30, -1e30, 1e30, -1e30), (1.0, -1.0, 0.25, 0.5), False),       # all four, far beyond
    ((-1e30, 0.5, -1e30, 1e30), (0.5, 0.25, 0.0, 0.5), False),
    ((0.5, 0.25, 0.75, 0.5), (1e30, 0.5, 0.25, -1e30), False),         # labels beyond the clamp
    ((0.5, -0.25, 100.0, 0.5), (0.25, 0.5, 0.0, 0.25), False),         # t2 = 100 (not clamped: keeps its gradient) against g2 = 0
    ((0.5, -0.25, -100.0, 0.5), (0.25, 0.5, 0.0, 0.25), False),        # t2 = -100
    ((0.5, -0.25, 0.5, -100.0), (0.25, 0.5, 0.25, 100.0), False),      # t3 = -100 against g3 = 100
]
N_TIES = sum(1 for p in PALETTE if p[2])

# name, layout, classes, positives per sample, generator, confidence loss, gamma, alpha, loc_weight
#   classes 27 | 28: last of the narrow path (rows in registers) | first of the wide one; 127: 4 cells per workgroup
#   a count of 0: a sample without positives; a count of A: every anchor positive
CASES = [
    ('giou vgg300 mining', VGG300, 20, [40, 0], 'palette', 'mining', 2.0, 0.25, 1.0),
    ('giou vgg300 focal continuous', VGG300, 20, [7, 300], 'continuous', 'focal', 2.0, 0.25, 2.0),
    ('giou A 32256', BIG32, 20, [5000], 'palette', 'focal', 2.0, 0.5, 1.0),
    ('giou tiny mining', TINY, 20, [24, 0, 64, 30], 'palette', 'mining', 2.0, 0.25, 5.0),
    ('giou tiny focal 1 class', TINY, 1, [3, 64, 0], 'continuous', 'focal', 1.0, 0.25, 1.0),
    ('giou A 1024 nj 8', A1024, 20, [10, 100, 300], 'palette', 'mining', 2.0, 0.25, 0.5),
    ('giou A 1025', A1025, 20, [30, 0, 300], 'palette', 'focal', 0.5, 0.25, 1.0),
    ('giou 1 class', MID, 1, [20, 300, 700], 'palette', 'mining', 2.0, 0.25, 1.0),
    ('giou 27 classes mining', MID, 27, [20, 300, 2302], 'palette', 'mining', 2.0, 0.25, 2.0),
    ('giou 27 classes focal', MID, 27, [20, 0, 2302], 'continuous', 'focal', 2.0, 0.25, 1.0),
    ('giou 28 classes mining', MID, 28, [20, 300, 0], 'palette', 'mining', 2.0, 0.25, 1.0),
    ('giou 28 classes focal', MID, 28, [20, 1, 700], 'continuous', 'focal', 2.0, 0.75, 10.0),
    ('giou 127 classes mining', MID, 127, [20, 2302, 700], 'palette', 'mining', 2.0, 0.25, 1.0),
    ('giou 127 classes focal', MID, 127, [20, 300], 'continuous', 'focal', 1.0, 0.5, 2.0),
]
CASE_IDS = [c[0] for c in CASES]


def _draw(rng, n):
    """n separated (t, g) pairs, float32"""
    t = np.zeros((n, 4), np.float32); g = np.zeros((n, 4), np.float32)
    todo = np.arange(n)
    while len(todo):
        k = len(todo)
        gg = rng.normal(0, 1.5, (k, 4))
        tt = gg + rng.normal(0, 2.0, (k, 4))
        far = rng.random(k) < 1 / 3
        tt[far, :2] += rng.choice([-1.0, 1.0], (int(far.sum()), 2)) * rng.uniform(8, 40, (int(far.sum()), 2))
        t[todo] = tt.astype(np.float32); g[todo] = gg.astype(np.float32)
        todo = todo[~gr.separated(t[todo], g[todo])]
    return t, g


def make(name, layout, C_, pos_counts, kind):
    """(out [B,A,nv] f32, labels [B,A,nv] f32, tie [B,A] bool: the anchors that hold one of the palette's tie entries), seeded by
    the case's name"""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    A = lr.layout(*layout, C_)['A']
    out, y = lr.palette_batch(rng, A, C_, pos_counts) if kind == 'palette' else lr.continuous_batch(rng, A, C_, pos_counts)
    nc = C_ + 1
    tie = np.zeros(y.shape[:2], bool)
    for b in range(len(pos_counts)):
        idx = np.flatnonzero(y[b, :, nc - 1] == 0)
        t, g = _draw(rng, len(idx))
        for i in range(min(len(idx), len(PALETTE))):
            pt, pg, is_tie = PALETTE[(i + 5 * b) % len(PALETTE)]
            t[i] = pt; g[i] = pg
            tie[b, idx[i]] = is_tie
        out[b, idx, nc:] = t
        y[b, idx, nc:] = g
    return out, y, tie
