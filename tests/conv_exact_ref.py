"""numpy / float64 reference of the training convolutions (forward, data gradient, weight gradient) with TF geometry, and operands on
which every fp32 kernel must give the reference's value bit for bit.

Geometry is gpu_util.conv_geom's: 'SAME', 'VALID' and 'BR1' (tf.pad bottom / right by one, then VALID); tensors are NHWC, filters HWIO.
Every function returns the value next to `absacc`, the same sum over the magnitudes of its products (as mxfp6_ref.conv_values does).

Exact operands (`operands`): every value is i * 2^s with a small integer i and a small exponent s >= 0 that vary with batch, row,
column, channel, 32-channel block, tap and output channel, asymmetric in each of them; x (which is also the relu mask of the data
gradient) and prev hold exact zeros and negative values, the bias is integer, the weight decay is 0.25.  A case is admissible when
every value is a multiple of one power of two (LSB, the weight decay's 2^-2) and every sum of magnitudes, taken in any order, stays
below 2^24 LSB: then no partial sum of any kernel rounds in fp32, whatever its order, split or tile.  `operands` lowers the exponent
ranges per case until `admissible` holds and asserts it."""
import numpy as np

WD = 0.25
LSB = 0.25                       # of every value: operands are integers, wd * w is a multiple of 1/4
# exponent spans (x, w, dy), tried from the widest down
SPANS = [(3, 2, 2), (2, 2, 2), (2, 1, 1), (1, 1, 1), (1, 1, 0), (1, 0, 0), (0, 0, 0)]


class Geom:
    def __init__(self, b, hi, wi, ci, co, k, stride, dil, padding):
        self.b, self.hi, self.wi, self.ci, self.co, self.kh, self.kw, self.stride, self.dil = b, hi, wi, ci, co, k, k, stride, dil
        self.ph, self.pw, self.ho, self.wo = geometry(hi, wi, k, stride, dil, padding)

    def replace(self, **kw):
        g = Geom.__new__(Geom)
        g.__dict__.update(self.__dict__)
        g.__dict__.update(kw)
        return g

    def abi(self):
        """the C ABI's geometry arguments"""
        return (self.b, self.hi, self.wi, self.ci, self.ho, self.wo, self.co, self.kh, self.kw, self.stride, self.dil, self.ph, self.pw)


def geometry(hi, wi, k, stride, dil, padding):
    """(pad_h, pad_w, ho, wo): TF's SAME puts the odd cell of padding at the bottom / right"""
    keff = (k - 1) * dil + 1
    if padding == 'SAME':
        ho, wo = -(-hi // stride), -(-wi // stride)
        return max((ho - 1) * stride + keff - hi, 0) // 2, max((wo - 1) * stride + keff - wi, 0) // 2, ho, wo
    extra = {'VALID': 0, 'BR1': 1}[padding]
    return 0, 0, (hi + extra - keff) // stride + 1, (wi + extra - keff) // stride + 1


def _rows(n_out, n_in, stride, pad, off):
    """input index of every output index for one tap offset; -> (indices of the outputs that land inside, their input indices)"""
    i = np.arange(n_out) * stride - pad + off
    ok = (i >= 0) & (i < n_in)
    return np.nonzero(ok)[0], i[ok]


def _taps(g):
    for r in range(g.kh):
        oh, ih = _rows(g.ho, g.hi, g.stride, g.ph, r * g.dil)
        for s in range(g.kw):
            ow, iw = _rows(g.wo, g.wi, g.stride, g.pw, s * g.dil)
            if len(oh) and len(ow):
                yield r, s, oh[:, None], ow[None, :], ih[:, None], iw[None, :]


def _conv(x, w, g):
    acc = np.zeros((g.b, g.ho, g.wo, g.co))
    for r, s, oh, ow, ih, iw in _taps(g):
        acc[:, oh, ow] += x[:, ih, iw] @ w[r, s]
    return acc


def _conv_t(dy, w, g):
    dx = np.zeros((g.b, g.hi, g.wi, g.ci))
    for r, s, oh, ow, ih, iw in _taps(g):
        dx[:, ih, iw] += dy[:, oh, ow] @ w[r, s].T
    return dx


def _corr(x, dy, g):
    dw = np.zeros((g.kh, g.kw, g.ci, g.co))
    for r, s, oh, ow, ih, iw in _taps(g):
        dw[r, s] = x[:, ih, iw].reshape(-1, g.ci).T @ dy[:, oh, ow].reshape(-1, g.co)
    return dw


def f64(a):
    return np.asarray(a, np.float64)


def forward(x, w, bias, relu, g, absacc=True):
    """-> (relu?(conv(x, w) + bias), absacc = conv(|x|, |w|))"""
    x, w = f64(x), f64(w)
    y = _conv(x, w, g) + f64(bias)
    return (np.maximum(y, 0.0) if relu else y), (_conv(np.abs(x), np.abs(w), g) if absacc else None)


def dgrad(dy, w, g, prev=None, mask=None, mask_ge=False, absacc=True):
    """-> (dx or (prev + dx) * (mask > 0), absacc of dx's products).  mask_ge: the wrong mask (>= 0), for the sensitivity checks"""
    dy, w = f64(dy), f64(w)
    dx = _conv_t(dy, w, g)
    if prev is not None:
        dx = dx + f64(prev)
    if mask is not None:
        dx = dx * ((f64(mask) >= 0) if mask_ge else (f64(mask) > 0))
    return dx, (_conv_t(np.abs(dy), np.abs(w), g) if absacc else None)


def wgrad(x, dy, w, wd, g, absacc=True):
    """-> (dw + wd * w, db, absacc of dw's products, absacc of db)"""
    x, dy = f64(x), f64(dy)
    return (_corr(x, dy, g) + wd * f64(w), dy.sum((0, 1, 2)), _corr(np.abs(x), np.abs(dy), g) if absacc else None,
            np.abs(dy).sum((0, 1, 2)))


def bf16_round(a):
    """float64 / float32 values that fp32 holds exactly -> nearest bf16, ties to even, as float64"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


# ---- operands ------------------------------------------------------------------------------------------------------------------------

def pattern(shape, mul, lo, n, span, image=False):
    """[b][h][w][c] values i * 2^s: i in lo ... lo + n - 1, s in 0 ... span; image: integers 0 ... 255"""
    B, H, W, C = np.meshgrid(*[np.arange(s) for s in shape], indexing='ij')
    blk = C // 32
    m = mul
    if image:
        return ((37 * B + 13 * H + 29 * W + 71 * C + 5 * ((H * W) % 17) + 3 * ((B * H) % 5)) % 256).astype(np.float64)
    i = (m[0] * B + m[1] * H + m[2] * W + m[3] * C + (H * C) % 3 + (W * blk) % 5 + (H * W) % 7 + 2 * blk + (B * W) % 2) % n + lo
    s = (2 * B + 3 * H + W + 2 * blk + (H * blk) % 3 + (W * C) % 2) % (span + 1)
    return np.ldexp(i.astype(np.float64), s)


def _filter(k, ci, co, span):
    KH, KW, CI, CO = np.meshgrid(np.arange(k), np.arange(k), np.arange(ci), np.arange(co), indexing='ij')
    blk = CI // 32
    j = (2 * KH + 3 * KW + CI + 7 * CO + (CI * CO) % 3 + (KH * CI) % 2 + blk + (KW * CO) % 5) % 7 - 3
    t = (KH * k + KW + 2 * CO + 3 * blk + (CO * blk) % 3 + (CI * KW) % 2) % (span + 1)
    return np.ldexp(j.astype(np.float64), t)


def real_columns(co):
    """the fused multibox heads pad 4 / 6 box types x 25 outputs to a multiple of 8: the padding columns are zero in the product"""
    return {152: 150, 104: 100}.get(co, co)


class Operands:
    pass


def make_operands(g, spans, image):
    sx, sw, sd = spans
    o = Operands()
    o.g, o.spans, o.wd = g, spans, WD
    o.x = pattern((g.b, g.hi, g.wi, g.ci), (5, 3, 7, 1), -3, 11, sx, image)
    o.w = _filter(g.kh, g.ci, g.co, sw)
    o.bias = ((5 * np.arange(g.co) + (np.arange(g.co) // 3) % 4) % 17 - 8).astype(np.float64)
    n = real_columns(g.co)
    o.w[..., n:] = 0
    o.bias[n:] = 0
    o.dy = pattern((g.b, g.ho, g.wo, g.co), (3, 5, 2, 1), -4, 9, sd)
    # the pattern's column sums over whole periods barely depend on the channel: one pixel of image 0 per channel carries a value of
    # the channel's own (-56 ... 56: seven bits, a bf16 value), so that the bias gradient tells the channels apart
    c = np.arange(g.co)
    o.dy.reshape(g.b, g.ho * g.wo, g.co)[0, (3 * c) % (g.ho * g.wo), c] = (c % 113) - 56
    o.prev = pattern((g.b, g.hi, g.wi, g.ci), (7, 2, 3, 5), -5, 13, sx)
    o.mask = o.x if not image else pattern((g.b, g.hi, g.wi, g.ci), (5, 3, 7, 1), -3, 11, 0)
    return o


def admissible(o, relu):
    """the exactness condition; -> None or the reason it fails.  Fills o.y, o.dx, o.dxm, o.dw, o.db (float64 expectations)."""
    g = o.g
    o.y, ay = forward(o.x, o.w, o.bias, relu, g)
    o.dx, adx = dgrad(o.dy, o.w, g)
    o.dxm = (o.dx + o.prev) * (o.mask > 0)
    o.dw, o.db, adw, adb = wgrad(o.x, o.dy, o.w, o.wd, g)
    sums = {'forward': ay + np.abs(o.bias), 'data gradient': adx + np.abs(o.prev), 'weight gradient': adw + np.abs(o.wd * o.w),
            'bias gradient': adb}
    for name, a in sums.items():
        if a.max() / LSB >= 2 ** 24:
            return f'{name}: sum of magnitudes {a.max():.0f} is not below 2^24 LSB'
    for name, v in dict(x=o.x, w=o.w, bias=o.bias, dy=o.dy, prev=o.prev, y=o.y, dx=o.dx, dxm=o.dxm, dw=o.dw, db=o.db, **sums).items():
        if not np.array_equal(np.round(v / LSB) * LSB, v):
            return f'{name} is not in multiples of {LSB}'
    return None


def distinct_enough(v):
    """more than 50 distinct values (a tensor of fewer than 100 elements: more than half as many as it has)"""
    return len(np.unique(v)) > min(50, v.size // 2)


def operands(case, image=False):
    """case = (name, b, hi, wi, ci, co, k, stride, dil, padding, relu, ...) -> Operands with the expectations filled in"""
    name, b, hi, wi, ci, co, k, stride, dil, padding, relu = case[:11]
    g = Geom(b, hi, wi, ci, co, k, stride, dil, padding)
    why = None
    for spans in SPANS:
        o = make_operands(g, spans, image)
        why = admissible(o, relu)
        if why is None:
            break
    assert why is None, f'{name}: {why}'
    o.name, o.relu = name, bool(relu)
    for n in ('y', 'dx', 'dxm', 'dw', 'db'):
        assert distinct_enough(getattr(o, n)), f'{name}: {n} takes {len(np.unique(getattr(o, n)))} distinct values'
    for n in ('mask', 'prev') + (() if image else ('x',)):
        v = getattr(o, n)
        assert (v == 0).any() and (v < 0).any() and (v > 0).any(), f'{name}: {n} needs zeros and both signs'
    return o


# the shapes the exact tests add to the kernels' own case lists: (name, b, hi, wi, ci, co, k, stride, dil, padding, relu)
EXTRA_CASES = [
    ('M below one tile 1x3x2 64->64', 1, 3, 2, 64, 64, 3, 1, 1, 'SAME', True),
    ('M one pixel over a 128-row tile 1x3x43 64->128', 1, 3, 43, 64, 128, 3, 1, 1, 'SAME', True),
    ('8 output channels 2x9x7 64->8', 2, 9, 7, 64, 8, 3, 1, 1, 'SAME', False),
    ('three k-chunks, the last partial 2x7x5 136->64', 2, 7, 5, 136, 64, 3, 1, 1, 'SAME', True),
]
