"""numpy float64 oracle of gradient clipping by global norm (include/ssdvgg_hip.h "gradient clipping") and the
operands and cases its tests share (test_clip_ref.py on the CPU, test_gpu_grad_clip.py on the GPU).

    S = sum (double)g[i]^2;  norm = |s| * sqrt(S);  f = 1 if norm <= max_norm else max_norm / norm (fp64, rounded to float once);
    S not finite: the update is skipped, f = 0.
"""
import functools
import os
import re

import numpy as np

# The launcher's shape, read from the launcher (csrc/ops.h): 4-float groups one block takes per pass, blocks at most, and how many
# passes of the grid the norm kernel's main loop loads together (its one-pass loop takes what is left).  test_gpu_grad_clip.py
# checks the first two against ssd_op_grad_norm_ws_bytes as well.
def _launcher_constant(name):
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'ssd_tensorflow_amd', 'csrc', 'ops.h')).read()
    m = re.search(r'constexpr\s+int\s+%s\s*=\s*([0-9 *]+);' % name, text)
    assert m, name + ' is not in csrc/ops.h'
    return int(np.prod([int(f) for f in m.group(1).split('*')]))


GROUPS_PER_BLOCK = _launcher_constant('GRAD_NORM_BLOCK')
GRID_CAP = _launcher_constant('GRAD_NORM_GRID_CAP')
UNROLL = _launcher_constant('GRAD_NORM_UNROLL')
BLOCK_FLOATS = 4 * GROUPS_PER_BLOCK
GRID_FLOATS = BLOCK_FLOATS * GRID_CAP            # one pass of the full grid
MAIN_FLOATS = (UNROLL - 1) * GRID_FLOATS         # a thread enters the main loop when more than this lies behind its first group
# The smallest sizes that reach every boundary of the launcher and of the norm kernel's two loops: one group, two, a block's last
# lanes idle, one group short of / at / one group past one block's worth and one full grid's worth of one pass, a size whose second
# pass is one group long; then one group short of, at (the one-pass loop alone, UNROLL - 1 trips) and one group past (thread 0 alone
# takes the main loop, and its last load is the last group) the main loop's entry, one group past a whole main trip (main loop, then
# one trip of the one-pass loop), and one group past the main loop's second trip.
SIZES = (4, 8, 252, 1024, BLOCK_FLOATS - 4, BLOCK_FLOATS, BLOCK_FLOATS + 4, 2 ** 20 + 4, GRID_FLOATS - 4, GRID_FLOATS, GRID_FLOATS + 4,
         MAIN_FLOATS - 4, MAIN_FLOATS, MAIN_FLOATS + 4, UNROLL * GRID_FLOATS + 4, (2 * UNROLL - 1) * GRID_FLOATS + 4)
SIZES = tuple(dict.fromkeys(SIZES))
# (grad_scale, max_norm as a multiple of the oracle's norm): clipped, not clipped, measured only
SETTINGS = ((0.25, 0.5), (1.0, 2.0), (0.5, float('inf')))
LR, MOMENTUM = np.float32(1e-3), np.float32(0.9)


def sum_squares(g):
    g = np.asarray(g, np.float64)
    return float(np.sum(g * g))      # (numpy's pairwise fp64 sum: off by a few 2^-53 relative)


def norm(g, s):
    """fp64 norm of the scaled gradient; not finite where g has a NaN or an Inf"""
    with np.errstate(invalid='ignore', over='ignore'):
        return abs(float(np.float32(s))) * float(np.sqrt(np.float64(sum_squares(g))))


def skipped(g):
    with np.errstate(invalid='ignore', over='ignore'):
        return not np.isfinite(sum_squares(g))


def factor(g, s, max_norm):
    """float32 factor of the update"""
    if skipped(g):
        return np.float32(0.0)
    nv, m = norm(g, s), float(np.float32(max_norm))
    return np.float32(1.0) if nv <= m else np.float32(m / nv)


def update(w, acc, g, s, max_norm, lr=LR, momentum=MOMENTUM):
    """(w', acc', float32 norm, float32 factor): the optimizer's expression in float32 with gscale' = s * f, every bit kept when skipped.
    (numpy rounds the product and the sum apart where the GPU may fuse them: compare to rounding, not to the bit.)"""
    w, acc, g = (np.asarray(a, np.float32) for a in (w, acc, g))
    f = factor(g, s, max_norm)
    with np.errstate(invalid='ignore', over='ignore'):
        n32 = np.float32(norm(g, s))
    if skipped(g):
        return w.copy(), acc.copy(), n32, f
    gs = np.float32(s) * f
    a = momentum * acc + gs * g
    return w - lr * a, a, n32, f


def ulps(a, b):
    """distance of two finite float32 values in units in the last place"""
    i = np.array([a, b], np.float32).view(np.int32).astype(np.int64)
    i = np.where(i < 0, -(i & 0x7fffffff), i)
    return int(abs(i[0] - i[1]))


def heavy_groups(n):
    """the 4-float groups of operands(n) that sit at the top of the magnitude range: the first, the middle and the last one, and the first
    group of every pass of the full grid (what thread 0 loads: in the main loop they are its v[0] ... v[UNROLL - 1])"""
    n4 = n // 4
    return sorted({0, n4 // 2, n4 - 1} | set(range(0, n4, GRID_CAP * GROUPS_PER_BLOCK)))


@functools.lru_cache(maxsize=2)
def operands(n):
    """(w, acc, g) of n floats, read-only: g non-zero everywhere, of mixed sign, magnitudes spread over 2^-20 ... 2^20 (a float32 running sum
    of the squares drops most of them); heavy_groups(n) sit at the top of that range, so that a group lost, counted twice or taken from
    the wrong pass at an edge of a loop moves the norm by far more than an ulp.  w and acc non-zero."""
    rng = np.random.default_rng(1000 + n)
    mag = np.exp2(rng.uniform(-20.0, 20.0, n)) * rng.uniform(1.0, 2.0, n)
    for grp in heavy_groups(n):
        mag[4 * grp:4 * grp + 4] = np.exp2(20.0) * rng.uniform(1.0, 2.0, 4)
    sign = rng.choice([-1.0, 1.0], n)
    sign[0], sign[1] = 1.0, -1.0          # (both signs at every size)
    g = (mag * sign).astype(np.float32)
    w = (rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    acc = (rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    for a in (w, acc, g):
        a.setflags(write=False)
    return w, acc, g


def max_norm_of(n, s, rel):
    """the float32 threshold of a case: rel x the oracle's norm of operands(n) under grad_scale s"""
    return np.float32(rel * norm(operands(n)[2], s))


# every setting at every size up to one pass past the main loop's entry; the two sizes beyond it (64 and 112 MB a buffer) take the
# clipping one alone
CASES = [(n, s, rel) for n in SIZES for s, rel in (SETTINGS if n <= MAIN_FLOATS + 4 else SETTINGS[:1])]
CASE_IDS = ['n%d-s%g-x%g' % c for c in CASES]
