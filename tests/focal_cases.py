"""The inputs of the focal-loss op tests, shared by test_gpu_focal.py (which runs them through the kernels) and test_focal_ref.py
(which shows on the same inputs that each seeded mistake of focal_ref.py moves the results by far more than the GPU bounds).

Layouts are those of test_gpu_loss.py (restated).  Inputs come from loss_ref.palette_batch (saturated rows: cross entropy exactly
0 in fp32) and loss_ref.continuous_batch.  `easy` names one sample whose background anchors are overwritten by nearly saturated
rows (every class logit 0, the background logit 14, 15 or 16: cross entropies of 1e-5 .. 1e-6 at 20 classes), the input on which
1 - exp(-ce) in place of -expm1(-ce) loses its digits."""
import zlib

import numpy as np

import loss_ref as lr

VGG300 = lr.PRESET_LAYOUTS['vgg300']
BIG32 = ([64 * 64, 32 * 32, 16 * 16], [6, 6, 6])                     # A = 32256: focal_sample_kernel<32>
TINY = ([9, 4, 1], [4, 6, 4])                                        # A = 64: most threads hold no anchor
A1024 = ([128], [8])                                                 # every thread of the sample kernel holds one anchor; nj = 8
A1025 = ([128, 1], [8, 1])                                           # ... and thread 0 a second one
MID = ([361, 100, 25, 9, 1], [4, 6, 8, 6, 4])                        # A = 2302, ragged cell chunks, nj = 8 on one map

# name, layout, classes, positives per sample, generator, gamma, alpha, easy sample (or None)
#   classes 27 | 28: last of the narrow path (rows in registers) | first of the wide one; 127: 4 cells per workgroup
#   a count of 0: a sample without positives; a count of A: every anchor positive
CASES = [
    ('vgg300 with a sample without positives', VGG300, 20, [40, 0], 'palette', 2.0, 0.25, None),
    ('vgg300 continuous', VGG300, 20, [7, 300], 'continuous', 0.5, 0.75, None),
    ('A 32256 (template 32)', BIG32, 20, [5000], 'palette', 5.0, 0.5, None),
    ('tiny: no positives, all positive', TINY, 20, [3, 0, 64, 1], 'palette', 0.0, 0.5, None),
    ('tiny 1 class continuous', TINY, 1, [3, 64, 0], 'continuous', 1.0, 0.25, None),
    ('A 1024 nj 8', A1024, 20, [10, 100, 300], 'palette', 1.0, 0.75, None),
    ('A 1025', A1025, 20, [10, 0, 300], 'palette', 0.5, 0.25, None),
    ('1 class', MID, 1, [20, 300, 700], 'palette', 2.0, 0.75, None),
    ('27 classes (last narrow)', MID, 27, [20, 300, 700], 'palette', 0.5, 0.5, None),
    ('27 classes gamma 0', MID, 27, [20, 0, 2302], 'continuous', 0.0, 0.25, None),
    ('28 classes (first wide)', MID, 28, [20, 300, 0], 'palette', 2.0, 0.25, None),
    ('28 classes continuous', MID, 28, [20, 1, 700], 'continuous', 5.0, 0.75, None),
    ('127 classes', MID, 127, [20, 2302, 700], 'palette', 0.5, 0.25, None),
    ('127 classes continuous', MID, 127, [20, 300], 'continuous', 1.0, 0.5, None),
    ('easy sample gamma 2', MID, 20, [20, 0, 700], 'palette', 2.0, 0.25, 1),
    ('easy sample gamma 5', TINY, 20, [0, 3], 'palette', 5.0, 0.75, 0),
]
CASE_IDS = [c[0] for c in CASES]
EASY_LEADS = np.array([14.0, 15.0, 16.0], np.float32)


def make(name, layout, C_, pos_counts, kind, easy=None):
    """(out [B,A,nv] f32, labels [B,A,nv] f32), seeded by the case's name"""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    A = lr.layout(*layout, C_)['A']
    out, y = lr.palette_batch(rng, A, C_, pos_counts) if kind == 'palette' else lr.continuous_batch(rng, A, C_, pos_counts)
    if easy is not None:
        nc = C_ + 1
        neg = y[easy, :, nc - 1] != 0
        out[easy, neg, :nc - 1] = 0.0
        out[easy, neg, nc - 1] = EASY_LEADS[rng.integers(0, len(EASY_LEADS), int(neg.sum()))]
    return out, y
