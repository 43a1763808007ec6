"""numpy restatement of csrc/winograd.hip's algorithm -- F(4x4, 3x3) on the interpolation points 0, +-3/4, +-3/2, inf -- in fp32, to
measure what the ALGORITHM loses against float64, and the error measure the GPU test shares with it.

    rho = max over elements of |got - ref64| / (2^-24 * A),   A = the same sum as ref64 over the operands' magnitudes
    (forward: conv(|x|, |w|) + |bias|; data gradient: conv^T(|dy|, |w|) (+ |prev|); weight gradient: corr(|x|, |dy|) + |wd * w|;
    bias gradient: sum |dy|)

The filter transform divides by powers of 3, so no operands make this form exact; the GPU test (tests/test_gpu_wino_bound.py) asserts
rho_gpu <= 2 * rho_emul per pass and case instead, the factor 2 for another association inside the transforms and split accumulators.
The restatement is the least favourable order a kernel would use: every transform row is a left-to-right fp32 sum, products are
rounded before they are added (no fma), and the channel sum (forward, data gradient) and the tile sum (weight gradient) run
sequentially in fp32 -- numpy's pairwise sum would flatter it.  Dilation d: every residue class (h mod d, w mod d) is an undilated
image of its own, as in the kernel.  The matrices are the kernel's (bt6, at4, a6, g6, gt3); dtype=np.float64 turns the same code into
the exact identity (tests/test_wino_emul.py)."""
import zlib
from fractions import Fraction as Fr

import numpy as np

import conv_exact_ref as cx


def _m(rows):
    return [[Fr(v) for v in r] for r in rows]


BT = _m([[Fr(81, 64), 0, Fr(-45, 16), 0, 1, 0],
         [0, Fr(-27, 16), Fr(-9, 4), Fr(3, 4), 1, 0],
         [0, Fr(27, 16), Fr(-9, 4), Fr(-3, 4), 1, 0],
         [0, Fr(-27, 32), Fr(-9, 16), Fr(3, 2), 1, 0],
         [0, Fr(27, 32), Fr(-9, 16), Fr(-3, 2), 1, 0],
         [0, Fr(81, 64), 0, Fr(-45, 16), 0, 1]])
G = _m([[Fr(64, 81), 0, 0],
        [Fr(-128, 243), Fr(-32, 81), Fr(-8, 27)],
        [Fr(-128, 243), Fr(32, 81), Fr(-8, 27)],
        [Fr(32, 243), Fr(16, 81), Fr(8, 27)],
        [Fr(32, 243), Fr(-16, 81), Fr(8, 27)],
        [0, 0, 1]])
AT = _m([[1, 1, 1, 1, 1, 0],
         [0, Fr(3, 4), Fr(-3, 4), Fr(3, 2), Fr(-3, 2), 0],
         [0, Fr(9, 16), Fr(9, 16), Fr(9, 4), Fr(9, 4), 0],
         [0, Fr(27, 64), Fr(-27, 64), Fr(27, 8), Fr(-27, 8), 1]])
BIAS_C = [Fr(-7, 9), Fr(14, 9), Fr(2, 9), 0, 0, Fr(7, 16)]           # c^T A = 1^T: the bias gradient from the transformed dy


def _t(m):
    return [list(r) for r in zip(*m)]


def _lin(mat, a, axis, dtype):
    """out[k] = sum_j mat[k][j] * a[j] along `axis`, left to right in `dtype`, the constants rounded to `dtype` first"""
    a = np.moveaxis(a, axis, 0)
    out = []
    for row in mat:
        acc = None
        for j, c in enumerate(row):
            if c == 0:
                continue
            t = a[j] if c == 1 else dtype(float(c)) * a[j]
            acc = t if acc is None else acc + t
        out.append(acc)
    out = np.stack(out)
    assert out.dtype == dtype
    return np.moveaxis(out, 0, axis)


def _two(mat, a, dtype):
    """mat . a . mat^T over the two axes in front of the channels: [..., n, n, C] -> [..., m, m, C]"""
    return _lin(mat, _lin(mat, a, -3, dtype), -2, dtype)


def _patches(x, lead, size):
    """[B, H, W, C] -> [B, th, tw, size, size, C]: tile (i, j) covers rows 4 i - lead ... 4 i - lead + size - 1, zero outside"""
    b, h, w, c = x.shape
    th, tw = -(-h // 4), -(-w // 4)
    xp = np.zeros((b, 4 * th + size - 4, 4 * tw + size - 4, c), x.dtype)
    xp[:, lead:lead + h, lead:lead + w] = x
    r = (4 * np.arange(th))[:, None] + np.arange(size)[None, :]
    s = (4 * np.arange(tw))[:, None] + np.arange(size)[None, :]
    return xp[:, r[:, None, :, None], s[None, :, None, :]]


def _classes(h, w, dil):
    return [(slice(r, h, dil), slice(c, w, dil)) for r in range(min(dil, h)) for c in range(min(dil, w))]


def _conv(x, w, dil, dtype):
    """y = conv(x, w), 3x3 / stride 1 / SAME at dilation dil, without the bias: [B, H, W, Ci] . [3, 3, Ci, Co] -> [B, H, W, Co]"""
    x, w = np.asarray(x, dtype), np.asarray(w, dtype)
    ci, co = w.shape[2:]
    U = _two(G, w.reshape(3, 3, ci * co), dtype).reshape(36, ci, co)
    y = np.zeros(x.shape[:3] + (co,), dtype)
    for rs, cs in _classes(x.shape[1], x.shape[2], dil):
        xc = x[:, rs, cs]
        b, h, wd = xc.shape[:3]
        V = _two(BT, _patches(xc, 1, 6), dtype)                             # [B, th, tw, 6, 6, Ci]
        th, tw = V.shape[1:3]
        V = V.reshape(b * th * tw, 36, ci)
        M = np.zeros((V.shape[0], 36, co), dtype)
        for k in range(ci):                                                 # the channel sum, one channel after another
            M = M + V[:, :, k, None] * U[None, :, k, :]
        o = _two(AT, M.reshape(b, th, tw, 6, 6, co), dtype)                 # [B, th, tw, 4, 4, Co]
        y[:, rs, cs] = o.transpose(0, 1, 3, 2, 4, 5).reshape(b, 4 * th, 4 * tw, co)[:, :h, :wd]
    return y


def forward(x, w, bias, relu, dil=1, dtype=np.float32):
    y = _conv(x, w, dil, dtype) + np.asarray(bias, dtype)
    return np.maximum(y, dtype(0)) if relu else y


def dgrad(dy, w, dil=1, prev=None, mask=None, dtype=np.float32):
    """the forward's three steps on dy with the filter rotated by 180 degrees and transposed; (prev + dx) * (mask > 0)"""
    wf = np.ascontiguousarray(np.asarray(w)[::-1, ::-1].transpose(0, 1, 3, 2))
    dx = _conv(dy, wf, dil, dtype)
    if prev is not None:
        dx = dx + np.asarray(prev, dtype)
    if mask is not None:
        dx = dx * (np.asarray(mask) > 0)
    return dx.astype(dtype)


def wgrad(x, dy, w, wd, dil=1, dtype=np.float32):
    """dU_p = sum over tiles of V_p^T (A dy A^T)_p, one tile after another; dw = G^T dU G + wd * w; db from the transformed dy"""
    x, dy, w = np.asarray(x, dtype), np.asarray(dy, dtype), np.asarray(w, dtype)
    ci, co = w.shape[2:]
    dU = np.zeros((36, ci, co), dtype)
    bs = np.zeros((36, co), dtype)
    for rs, cs in _classes(x.shape[1], x.shape[2], dil):
        V = _two(BT, _patches(x[:, rs, cs], 1, 6), dtype).reshape(-1, 36, ci)
        Ya = _two(_t(AT), _patches(dy[:, rs, cs], 0, 4), dtype).reshape(-1, 36, co)
        for t in range(V.shape[0]):
            dU = dU + V[t][:, :, None] * Ya[t][:, None, :]
            bs = bs + Ya[t]
    dw = _two(_t(G), dU.reshape(6, 6, ci * co), dtype).reshape(3, 3, ci, co) + dtype(wd) * w
    db = np.zeros((co,), dtype)
    for k in range(6):
        for l in range(6):
            if BIAS_C[k] != 0 and BIAS_C[l] != 0:
                db = db + (dtype(float(BIAS_C[k])) * dtype(float(BIAS_C[l]))) * bs[k * 6 + l]
    return dw, db


def rho(got, ref64, absacc):
    """max |got - ref64| / (2^-24 * A) over the elements with A > 0 (A = 0: the value must be exactly 0)"""
    err = np.abs(np.asarray(got, np.float64) - ref64)
    assert np.all(err[absacc == 0] == 0)
    return float((err[absacc > 0] / (2.0 ** -24 * absacc[absacc > 0])).max())


# ---- the cases and inputs the CPU measurement and the GPU test share ------------------------------------------------------------------

# (name, b, h, w, ci, co, dil): the small ones of test_gpu_winograd.CASES (the 19x19 dilation-6 layer with fewer channels)
CASES = [
    ('tiny 3x2 32->32 b5 (one tile per image)', 5, 3, 2, 32, 32, 1),
    ('exact tiles 8x12 128->96', 2, 8, 12, 128, 96, 1),
    ('dil 2 odd 13x9 64->64', 3, 13, 9, 64, 64, 2),
    ('mod_conv6 dil 6 19x19 64->96 (reduced channels)', 2, 19, 19, 64, 96, 6),
    ('12 output channels 9x9 32->12', 2, 9, 9, 32, 12, 1),
    ('128 -> 64 channels 21x10 (128 x 64 tile of the weight-gradient GEMM)', 2, 21, 10, 128, 64, 1),
]
PASSES = ('forward', 'dgrad', 'dgrad accumulate+mask', 'wgrad', 'wgrad, taps pooled', 'bias grad')
WD = 0.0005


class Inputs:
    pass


def inputs(case):
    """relu-like x, Gaussian filter / bias / dy as in test_gpu_winograd._run; dy masked by the layer's own relu; float64 references
    and the sums of magnitudes"""
    name, b, h, w, ci, co, dil = case
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    o = Inputs()
    o.g = cx.Geom(b, h, w, ci, co, 3, 1, dil, 'SAME')
    o.x = np.maximum(rng.normal(0, 1, (b, h, w, ci)), 0).astype(np.float32)
    o.w = (rng.normal(0, 1, (3, 3, ci, co)) / np.sqrt(9 * ci)).astype(np.float32)
    o.bias = rng.normal(0, 0.1, (co,)).astype(np.float32)
    dy = rng.normal(0, 1, (b, h, w, co)).astype(np.float32)
    o.prev = rng.normal(0, 1, o.x.shape).astype(np.float32)
    y, ay = cx.forward(o.x, o.w, o.bias, True, o.g)
    o.dy = (dy * (y > 0)).astype(np.float32)
    dx, adx = cx.dgrad(o.dy, o.w, o.g)
    dw, db, adw, adb = cx.wgrad(o.x, o.dy, o.w, np.float64(np.float32(WD)), o.g)
    o.ref = {'forward': (y, ay + np.abs(o.bias.astype(np.float64))), 'dgrad': (dx, adx),
             'dgrad accumulate+mask': ((dx + o.prev) * (o.x > 0), adx + np.abs(o.prev.astype(np.float64))),
             'wgrad': (dw, adw + np.abs(np.float64(np.float32(WD)) * o.w)), 'bias grad': (db, adb)}
    # the inverse transform G^T dU G mixes the nine taps of a (ci, co) pair: the same errors against A summed over the taps
    o.ref['wgrad, taps pooled'] = (dw, np.broadcast_to(o.ref['wgrad'][1].sum((0, 1), keepdims=True), dw.shape))
    return o


def emulate(o, dtype=np.float32):
    """-> {pass: tensor} of the restatement on the inputs o"""
    dil = o.g.dil
    dw, db = wgrad(o.x, o.dy, o.w, np.float32(WD), dil, dtype)
    return {'forward': forward(o.x, o.w, o.bias, True, dil, dtype), 'dgrad': dgrad(o.dy, o.w, dil, dtype=dtype),
            'dgrad accumulate+mask': dgrad(o.dy, o.w, dil, o.prev, o.x, dtype), 'wgrad': dw, 'wgrad, taps pooled': dw, 'bias grad': db}


def rho_emul(o):
    e = emulate(o)
    return {p: rho(e[p], *o.ref[p]) for p in PASSES}


def read_profile(path):
    """profiles/wino_error_bound.txt -> {(case name, pass): rho_emul}"""
    out = {}
    for line in open(path):
        if line.startswith('#') or not line.strip():
            continue
        name, p, v = line.rstrip('\n').split('\t')
        out[name, p] = float(v)
    return out


if __name__ == '__main__':      # python tests/wino_emul.py > profiles/wino_error_bound.txt
    print('# rho_emul = max |emulation - float64| / (2^-24 * sum of magnitudes): tests/wino_emul.py, fp32 numpy restatement of')
    print('# csrc/winograd.hip (F(4x4, 3x3), points 0, +-3/4, +-3/2, inf; sequential fp32 channel / tile sums) on the inputs of')
    print('# tests/test_gpu_wino_bound.py, which asserts rho_gpu <= 2 * rho_emul.  Columns: case, pass, rho_emul (tab-separated).')
    for c in CASES:
        for p, v in rho_emul(inputs(c)).items():
            print(f'{c[0]}\t{p}\t{v:.6g}')
