"""numpy oracle of the AdamW update (include/ssdvgg_hip.h "update rule") and the operands and cases its tests share
(test_adamw_ref.py on the CPU, test_gpu_adamw.py and test_gpu_adamw_model.py on the GPU).

The contract rounds every fp32 operation once, in the order written, with no fused multiply-add, an IEEE division and a correctly
rounded square root.  numpy's float32 arithmetic is exactly that, so `adamw` below is held to the BIT.  The host scalars are made
from np.float32 hyper-parameters through Python doubles and math.pow, as the library makes them in C doubles:

    gs  = gscale * g                        omb1 = f32(1 - b1)         omb2 = f32(1 - b2)
    m'  = (b1 * m) + (omb1 * gs)            rs2  = f32(1 / sqrt(1 - b2^t))
    v'  = (b2 * v) + (omb2 * (gs * gs))     ss   = f32(lr / (1 - b1^t))
    den = (sqrt(v') * rs2) + eps            ld   = f32(lr * decay)
    u   = m' / den
    x   = w - (ld * w) in front of n_decay, w behind it
    w'  = x - (ss * u)
"""
import collections
import functools
import math
import os
import re

import numpy as np

F = np.float32


def _launcher_constant(name):
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'ssd_tensorflow_amd', 'csrc', 'ops.h')).read()
    m = re.search(r'constexpr\s+int\s+%s\s*=\s*([0-9 *]+);' % name, text)
    assert m, name + ' is not in csrc/ops.h'
    return int(np.prod([int(f) for f in m.group(1).split('*')]))


# The launcher's shape, read from the launcher (csrc/ops.h): threads of a block (one 4-float group each per trip) and blocks at most
BLOCK = _launcher_constant('ADAMW_BLOCK')
GRID_CAP = _launcher_constant('ADAMW_GRID_CAP')
G = 4 * BLOCK * GRID_CAP            # floats of one pass of the full grid

Hyper = collections.namedtuple('Hyper', 'lr b1 b2 eps decay')
Scalars = collections.namedtuple('Scalars', 'b1 omb1 b2 omb2 rs2 eps ld ss')
DEFAULT = Hyper(F(1e-3), F(0.9), F(0.999), F(1e-8), F(0.01))


def hyper(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, decay=0.01):
    return Hyper(*(F(x) for x in (lr, b1, b2, eps, decay)))


def host_scalars(hp, t):
    """what the host derives in double from the float32 hyper-parameters and the count t >= 1, each rounded to float once"""
    lr, b1, b2, eps, decay = (float(F(x)) for x in hp)
    assert t >= 1
    return Scalars(b1=F(b1), omb1=F(1.0 - b1), b2=F(b2), omb2=F(1.0 - b2),
                   rs2=F(1.0 / math.sqrt(1.0 - math.pow(b2, float(t)))), eps=F(eps), ld=F(lr * decay),
                   ss=F(lr / (1.0 - math.pow(b1, float(t)))))


def adamw(w, m, v, g, n_decay, hp, t, gscale):
    """(w', m', v') in float32: the contract, one rounding per operation"""
    w, m, v, g = (np.asarray(a, F) for a in (w, m, v, g))
    a = host_scalars(hp, t)
    gs = F(gscale) * g
    mn = (a.b1 * m) + (a.omb1 * gs)
    vn = (a.b2 * v) + (a.omb2 * (gs * gs))
    den = (np.sqrt(vn) * a.rs2) + a.eps
    u = mn / den
    x = w.copy()
    x[:n_decay] = w[:n_decay] - (a.ld * w[:n_decay])
    wn = x - (a.ss * u)
    assert wn.dtype == mn.dtype == vn.dtype == F
    return wn, mn, vn


def adamw64(w, m, v, g, n_decay, hp, t, gscale):
    """the same expressions in float64 on the float32 operands and the float32 host scalars: what the float32 oracle rounds"""
    w, m, v, g = (np.asarray(a, np.float64) for a in (w, m, v, g))
    a = Scalars(*(float(x) for x in host_scalars(hp, t)))
    gs = float(F(gscale)) * g
    mn = a.b1 * m + a.omb1 * gs
    vn = a.b2 * v + a.omb2 * (gs * gs)
    u = mn / (np.sqrt(vn) * a.rs2 + a.eps)
    x = w.copy()
    x[:n_decay] *= 1.0 - a.ld
    return x - a.ss * u, mn, vn


@functools.lru_cache(maxsize=3)
def operands(n):
    """(w, m, v, g) of n floats, read-only.  g: magnitudes 2^-20 ... 2^20 of mixed sign, so that under the cases' scales no intermediate
    is subnormal (the smallest, omb2 * gs^2, is about 2^-54); m: O(1) of mixed sign; v >= 0 over 2^-30 ... 2^30; w: O(1) of mixed sign,
    none zero (so a decay in the wrong place shows).  Zeros of both signs sit in g and m and zeros in v, alone and together, in the first
    groups and the last one."""
    rng = np.random.default_rng(3500 + n)
    g = (np.exp2(rng.uniform(-20.0, 20.0, n)) * rng.uniform(1.0, 2.0, n) * rng.choice([-1.0, 1.0], n)).astype(F)
    m = (rng.uniform(0.25, 2.0, n) * rng.choice([-1.0, 1.0], n)).astype(F)
    v = (np.exp2(rng.uniform(-30.0, 30.0, n)) * rng.uniform(1.0, 2.0, n)).astype(F)
    w = (rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)).astype(F)
    g[0] = abs(g[0]); g[min(1, n - 1)] = -abs(g[min(1, n - 1)])
    if n >= 8:
        g[2], g[3] = 0.0, -0.0                  # a zero gradient: u = m' / den moves w by the old momentum alone
        m[3], m[4] = -0.0, 0.0                  # both zero at 3
        v[3], v[5] = 0.0, 0.0                   # everything zero at 3: den = eps, u = 0
        m[n - 1], v[n - 2] = 0.0, 0.0
        g[n - 3] = -0.0
    for a in (w, m, v, g):
        a.setflags(write=False)
    return w, m, v, g


Case = collections.namedtuple('Case', 'n n_decay t b1 b2 s')
TS = (1, 2, 1000, 10 ** 7)
SMALL = (4, 8, 1020, 1024, 1028)


def decays(n):
    """0, 1, 6 (inside a group of four), n - 3 and n, where the arena has them"""
    return [d for d in dict.fromkeys((0, 1, 6, n - 3, n)) if 0 <= d <= n]


def _cases():
    out = []
    for k, n in enumerate(SMALL):
        for j, d in enumerate(decays(n)):
            out.append(Case(n, d, TS[(j + k) % 4], 0.9, 0.999, (1.0, 0.25)[(j + k) % 2]))
    out += [Case(1028, 6, t, 0.9, 0.999, 0.25) for t in TS]
    out += [Case(1028, 1025, t, b1, b2, 0.5) for t in (1, 2) for b1, b2 in ((0.0, 0.999), (0.9, 0.0), (0.0, 0.0))]
    # one group short of a pass of the full grid, the pass, one group past it (thread 0's second trip; the decay ends inside it), two
    # passes and a group
    out += [Case(G - 4, G - 7, 2, 0.9, 0.999, 1.0), Case(G, 6, 1000, 0.9, 0.999, 0.25), Case(G + 4, G + 1, 1, 0.9, 0.999, 0.25),
            Case(G + 4, 1, 10 ** 7, 0.9, 0.999, 1.0), Case(2 * G + 4, 2 * G + 4, 2, 0.9, 0.999, 0.5), Case(2 * G + 4, 0, 1000, 0.9, 0.999, 1.0)]
    return list(dict.fromkeys(out))


CASES = _cases()
CASE_IDS = ['n%d-d%d-t%d-b%g-%g-s%g' % c for c in CASES]
SMALL_CASES = [c for c in CASES if c.n <= 1028]


def case_hyper(c):
    return hyper(b1=c.b1, b2=c.b2)


def ulps(a, b):
    """largest distance of two finite float32 arrays in units in the last place"""
    i = np.stack([np.asarray(a, F), np.asarray(b, F)]).view(np.int32).astype(np.int64)
    i = np.where(i < 0, -(i & 0x7fffffff), i)
    return int(np.abs(i[0] - i[1]).max())
