"""numpy oracle of the weight EMA's update (include/ssdvgg_hip.h "weight EMA") and the operands and cases its tests
share (test_ema_ref.py on the CPU, test_gpu_ema.py and test_gpu_ema_model.py on the GPU).

The contract rounds every fp32 operation once, in the order written, with no fused multiply-add.  numpy's float32 arithmetic is
exactly that, so `ema` below is held to the BIT.  The host scalar is made from the np.float32 decay through Python doubles, as the
library makes it in C doubles; t is the count of EMA updates BEFORE this one:

    d    = min(decay, (1 + t) / (10 + t))       omd = f32(1 - d)
    diff = e - w
    e'   = e - (omd * diff)
"""
import collections
import functools
import os
import re

import numpy as np

F = np.float32


def _launcher_constant(name):
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'ssd_tensorflow_amd', 'csrc', 'ops.h')).read()
    m = re.search(r'constexpr\s+int\s+%s\s*=\s*([0-9 *]+);' % name, text)
    assert m, name + ' is not in csrc/ops.h'
    return int(np.prod([int(f) for f in m.group(1).split('*')]))


# The launcher's shape, read from the launcher (csrc/ops.h; the EMA kernels take the AdamW update's): threads of a block (one
# 4-float group each per trip) and blocks at most
BLOCK = _launcher_constant('ADAMW_BLOCK')
GRID_CAP = _launcher_constant('ADAMW_GRID_CAP')
G = 4 * BLOCK * GRID_CAP            # floats of one pass of the full grid


def host_decay(decay, t):
    """d, in double: the float32 decay, or the warm-up (1 + t) / (10 + t) while that is smaller"""
    assert t >= 0
    return min(float(F(decay)), (1.0 + float(t)) / (10.0 + float(t)))


def host_scalar(decay, t):
    """omd = f32(1 - d): what the host hands the kernel"""
    return F(1.0 - host_decay(decay, t))


def ema_parts(e, w, omd):
    """(diff, product, e') in float32 under a given omd: one rounding per operation"""
    e, w = np.asarray(e, F), np.asarray(w, F)
    diff = e - w
    prod = F(omd) * diff
    out = e - prod
    assert diff.dtype == prod.dtype == out.dtype == F
    return diff, prod, out


def ema(e, w, decay, t):
    """e' in float32: the contract"""
    return ema_parts(e, w, host_scalar(decay, t))[2]


def ema64(e, w, decay, t):
    """the same expressions in float64 on the float32 operands and the float32 host scalar: what the float32 oracle rounds;
    -> (diff, product, e')"""
    e, w = np.asarray(e, np.float64), np.asarray(w, np.float64)
    omd = float(host_scalar(decay, t))
    diff = e - w
    prod = omd * diff
    return diff, prod, e - prod


@functools.lru_cache(maxsize=3)
def operands(n):
    """(e, w) of n floats, read-only.  w: O(1) of mixed sign; e = w * (1 + r) with |r| over 2^-20 ... 2 of mixed sign, so e is of
    mixed sign against w too and e - w spans 2^-20 ... 2 relative to w.  The smallest product omd * diff is about 2^-10 * 2^-21: no
    intermediate is subnormal under any case's omd.  Exact ties e == w (the same bits) sit in the first and the last group of four:
    an ordinary number at 1 (at n = 4, where the two groups are one, the only tie); from n = 8 on -0 at 3 and +0 at n - 2; from
    n = 1020 on an ordinary number at n - 3 too.  Zeros that are no ties: e = -0 against w = +0 at n - 1 (n >= 8), and from n = 1020
    on w = -0 under an ordinary e at 9 and e = +0 over an ordinary w at 10.  The smallest sizes keep the other elements ordinary, so
    that every mistake of test_ema_ref.py shows in them."""
    # (the two smallest sizes have three and five ordinary elements, and the form d * e + (1 - d) * w agrees with the contract in
    # about every second element: their seeds are ones under which it shows under every scalar -- test_ema_ref.py checks it)
    rng = np.random.default_rng({4: 3708, 8: 3713}.get(n, 3700 + n))
    w = (rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)).astype(F)
    r = np.exp2(rng.uniform(-20.0, 1.0, n)) * rng.choice([-1.0, 1.0], n)
    # an average near zero under a weight of O(1), at the head of both groups of the smallest sizes: e - w is 63 (33) times e there, so
    # a host scalar that is off by 2^-16 of itself -- the warm-up against the decay at t = 8990 under 0.999 -- moves e' by many ulps
    r[0] = -(1.0 - 2.0 ** -6)
    if n >= 8:
        r[4] = -(1.0 + 2.0 ** -5)
    e = (w.astype(np.float64) * (1.0 + r)).astype(F)
    e[1] = w[1]
    if n >= 8:
        e[3] = w[3] = F(-0.0)
        e[n - 2] = w[n - 2] = F(0.0)
        e[n - 1], w[n - 1] = F(-0.0), F(0.0)
    if n >= 1020:
        e[n - 3] = w[n - 3]
        w[9] = F(-0.0)
        e[10] = F(0.0)
    e.setflags(write=False)
    w.setflags(write=False)
    return e, w


def ties(n):
    """indices where e and w hold the same bits"""
    return [1] if n < 8 else [1, 3, n - 2] + ([n - 3] if n >= 1020 else [])


Case = collections.namedtuple('Case', 'n decay t')
SIZES = (4, 8, 1020, 1024, 1028, G - 4, G, G + 4, 2 * G + 4)
# decay 0.9: (1 + t) / (10 + t) reaches 0.9 at t = 80, so 79 is the last update under the warm-up and 80 ... 10^7 run under the decay;
# decay 0.999: 8990 is the last under the warm-up (8991 / 9000 against the float32 0.999 = 0.99900001...); decay 0.5: t = 0 warms up
SCALARS = ((0.9, 0), (0.9, 1), (0.9, 79), (0.9, 80), (0.9, 89), (0.9, 90), (0.9, 10 ** 7), (0.999, 0), (0.999, 8990), (0.999, 8991), (0.5, 0))
WARM = {(0.9, 0), (0.9, 1), (0.9, 79), (0.999, 0), (0.999, 8990), (0.5, 0)}       # the warm-up is the smaller of the two


# every size under every scalar, by size (operands() keeps the last few).  The large sizes: one group short of a pass of the full grid,
# the pass, one group past it (thread 0's second trip), two passes and a group
CASES = [Case(n, d, t) for n in SIZES for d, t in SCALARS]
CASE_IDS = ['n%d-d%g-t%d' % c for c in CASES]
SMALL_CASES = [c for c in CASES if c.n <= 1028]


def ulps(a, b):
    """largest distance of two finite float32 arrays in units in the last place"""
    i = np.stack([np.asarray(a, F), np.asarray(b, F)]).view(np.int32).astype(np.int64)
    i = np.where(i < 0, -(i & 0x7fffffff), i)
    return int(np.abs(i[0] - i[1]).max())
