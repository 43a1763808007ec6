"""Plain numpy float64 references of the max-pool and L2-norm passes of csrc/ops.hip, the operands that make the pooling
expectations exact in fp32 and in bf16, and per-element error bounds for the L2 norm.  No torch in here.

Pooling.  `maxpool` scans a window kh-major, kw-minor; the first maximum wins; a cell outside the image never wins; the padding
in front of the image is explicit (TF SAME is one choice of it).  The gradient of a cell is the sum of the gradients of the
windows whose first maximum it is, plus the accumulated tensor if asked, and the relu mask zeroes that SUM wherever x > 0 is
false (-0.0 and 0.0 alike).  `record_2x2` / `rec_bwd` are the 12-bit record of the 2x2 stride-2 pools and the pass that reads
it, `arg_3x3` the tap record of the 3x3 stride-1 pool.  Every function takes `mutant`, one of MUTANTS: a reference that is wrong
in one way, for tests/test_pool_l2_ref.py to show that the operands tell right from wrong.

L2 norm over channels, y = scale * x * r with r = max(sum_c x^2, eps)^-1/2, eps = the fp32 value of 1e-12:
    dx = scale * g * r - x * k,  k = (sum_c scale * g * x) * r^3 where sum_c x^2 > eps, else 0;   dscale = sum_pix g * x * r.

The bounds, u = 2^-24 (half an fp32 ulp, relative), J = ceil(C / 256) chunks of 4 channels per lane, first order in u with the
fraction rounded up to cover the second-order terms:
  * the sum of squares has positive terms only, so its relative error is at most the number of roundings on its longest chain:
    1 for the product, 4 additions per chunk and lane (three inside the chunk, one into the lane's sum: 4J in all), 6 shuffle
    levels: (4J + 7) u.  A contraction into fma drops roundings and only lowers this.
  * r = rsqrtf(ss): half of that enters through the square root, (2J + 3.5) u; rsqrtf itself is within 1 ulp (the HIP
    programming guide's table of single-precision device functions), at most 2^-23 = 2 u relative:  RHO = 2J + 5.5.
  * forward, y = fl(fl(scale * x) * r): two multiplications,  K_f = RHO + 2 = 2J + 7.5 -> 2J + 8  (16 at J = 4, below 64):
        |y - y^| <= K_f u |y^|.
  * backward: t = sum_c scale * g * x has terms of both signs: 2 roundings per term, 4J + 6 additions, TAU = 4J + 8 against
    T = sum_c |scale * g * x|.  k = fl(fl(fl(t * r) * r) * r): |dk| <= r^3 T (TAU + 3 RHO + 3) u.  B = fl(x * k) adds one,
    A = fl(fl(scale * g) * r) has (RHO + 2) u |A|, the subtraction u (|A| + |B|) with |B| <= |x| r^3 T:
        |dx - dx^| <= K_b u (|scale g r| + |x| r^3 T),  K_b = TAU + 3 RHO + 5 = 10J + 29.5 -> 10J + 30.
  * dscale: a term fl(fl(g * x) * r) is within K_f u of its value; the terms are then added along a chain of K_chain additions
    (chain_length: the lane's pixel loop, the 4 waves of a workgroup, colsum_kernel's rows, pairs and 16 row groups), each
    addition one rounding of a partial sum that sum |g x r| bounds.  In the form of mxfp6_ref.accumulation_bound, one ulp per
    operation:   |ds - ds^| <= (K_chain + K_f) 2^-23 sum_pix |g x r|.
  * bf16 storage: the inputs are bf16 values and the reference is computed from them; the arithmetic is the fp32 one, and the
    store rounds once to nearest: a stored value is within half a bf16 ulp of the reference plus the fp32 bound (a computed
    value that crosses into the next binade lands on the power of two, within the fp32 bound)."""
import zlib

import numpy as np

MUTANTS = ('last_max', 'mask_ge', 'drop_accumulate', 'mask_before_accumulate', 'pad_shift', 'swap_khkw', 'reverse_fields',
           'positive_ge')
U = 2.0 ** -24
EPS = float(np.float32(1e-12))


# ---- pooling -----------------------------------------------------------------------------------------------------------------

def same_pad(n, k, s):
    """TF SAME: (leading pad, output size)"""
    out = -(-n // s)
    return max((out - 1) * s + k - n, 0) // 2, out


def _taps(k, mutant):
    """(tap number written to a record, kh, kw) in scan order"""
    if mutant == 'swap_khkw':
        return [(kw * k + kh, kh, kw) for kw in range(k) for kh in range(k)]
    return [(kh * k + kw, kh, kw) for kh in range(k) for kw in range(k)]


def _window_rows(n_out, stride, pad, kk, n_in):
    pos = np.arange(n_out) * stride - pad + kk
    return pos, (pos >= 0) & (pos < n_in)


def gather(x, k, stride, pad_h, pad_w, ho, wo, dy=None, mutant=None):
    """x [b][hi][wi][c] float64 -> (y [b][ho][wo][c], tap [b][ho][wo][c] = kh * k + kw of the first maximum, g [b][hi][wi][c] =
    per cell the sum of dy over the windows whose first maximum it is, or None)"""
    assert mutant is None or mutant in MUTANTS
    x = np.asarray(x, np.float64)
    b, hi, wi, c = x.shape
    if mutant == 'pad_shift':
        pad_h, pad_w = pad_h + 1, pad_w + 1          # (a window this leaves without a cell keeps -inf and tap 255)
    y = np.full((b, ho, wo, c), -np.inf)
    tap = np.full((b, ho, wo, c), 255, np.uint8)
    geom = []
    for t, kh, kw in _taps(k, mutant):
        hh, vh = _window_rows(ho, stride, pad_h, kh, hi)
        ww, vw = _window_rows(wo, stride, pad_w, kw, wi)
        if not vh.any() or not vw.any():
            continue
        sel = np.ix_(np.arange(b), np.flatnonzero(vh), np.flatnonzero(vw), np.arange(c))       # the windows that have this tap
        cells = np.ix_(np.arange(b), hh[vh], ww[vw], np.arange(c))                              # and the cell it is, one each
        geom.append((t, sel, cells))
        v, ysub, tsub = x[cells], y[sel], tap[sel]
        win = (v >= ysub) if mutant == 'last_max' else ((v > ysub) | (tsub == 255))
        y[sel] = np.where(win, v, ysub)
        tap[sel] = np.where(win, np.uint8(t), tsub)
    assert mutant == 'pad_shift' or (tap != 255).all(), 'a window without a cell inside the image'
    if dy is None:
        return y, tap, None
    g = np.zeros_like(x)
    dy = np.asarray(dy, np.float64)
    for t, sel, cells in geom:
        g[cells] += np.where(tap[sel] == t, dy[sel], 0.0)
    return y, tap, g


def maxpool(x, k, stride, pad_h, pad_w, ho, wo, dy=None, prev=None, accumulate=False, relu_mask=False, mutant=None):
    """-> (y, tap, dx): gather, then dx = the gathered gradient (+ prev if accumulate), zeroed where x > 0 is false if relu_mask"""
    y, tap, g = gather(x, k, stride, pad_h, pad_w, ho, wo, dy, mutant)
    return y, tap, None if g is None else finish_dx(g, np.asarray(x, np.float64), prev, accumulate, relu_mask, mutant)


def finish_dx(g, x, prev, accumulate, relu_mask, mutant=None):
    """the gathered gradient -> dx: + prev if accumulate, then the relu mask on the sum"""
    keep = (x >= 0) if mutant == 'mask_ge' else (x > 0)
    if relu_mask and mutant == 'mask_before_accumulate':
        g = np.where(keep, g, 0.0)
    if accumulate and mutant != 'drop_accumulate':
        g = g + np.asarray(prev, np.float64)
    if relu_mask and mutant != 'mask_before_accumulate':
        g = np.where(keep, g, 0.0)
    return g


def _fields(a, bits, mutant):
    """[..., c] small integers -> [..., c / 4] words, channel e of a group in bits bits * e ..."""
    a = a.reshape(a.shape[:-1] + (a.shape[-1] // 4, 4)).astype(np.uint32)
    order = (3, 2, 1, 0) if mutant == 'reverse_fields' else (0, 1, 2, 3)
    out = np.zeros(a.shape[:-1], np.uint32)
    for e in range(4):
        out |= a[..., e] << np.uint32(bits * order[e])
    return out


def record_2x2(x, mutant=None):
    """the record of maxpool2x2_fwd_rec_kernel: uint16 [b][ho][wo][c / 4]; channel e of a group: bits 3e, 3e + 1 = the first
    maximum's cell (0 = (h0, w0), 1 = (h0, w0 + 1), 2 = (h0 + 1, w0), 3 = (h0 + 1, w0 + 1)), bit 3e + 2 = "maximum > 0";
    the top 4 bits are zero"""
    b, hi, wi, c = x.shape
    ho, wo = (hi + 1) // 2, (wi + 1) // 2
    y, tap, _ = maxpool(x, 2, 2, 0, 0, ho, wo, mutant=mutant)
    pos = (y >= 0) if mutant == 'positive_ge' else (y > 0)
    rec = _fields(tap.astype(np.uint32) | (pos.astype(np.uint32) << np.uint32(2)), 3, mutant)
    assert (rec >> 12 == 0).all()
    return rec.astype(np.uint16)


def rec_bwd(rec, dy, relu_mask, hi, wi):
    """dx [b][hi][wi][c] of maxpool2x2_bwd_rec_kernel: every cell inside the image is written (nothing to accumulate)"""
    dy = np.asarray(dy, np.float64)
    b, ho, wo, c = dy.shape
    r = np.stack([(rec.astype(np.uint32) >> np.uint32(3 * e)) & 7 for e in range(4)], -1).reshape(b, ho, wo, c)
    dx = np.zeros((b, 2 * ho, 2 * wo, c))
    for q in range(4):
        hit = ((r & 3) == q) & ((r & 4) != 0 if relu_mask else True)
        dx[:, q >> 1::2, q & 1::2] = np.where(hit, dy, 0.0)
    return dx[:, :hi, :wi]


def arg_3x3(x, mutant=None):
    """the record of maxpool_taps_kernel<3> (3x3 stride 1 SAME): uint32 [b][h][w][c / 4], byte e = kh * 3 + kw of channel e"""
    b, hi, wi, c = x.shape
    _, tap, _ = maxpool(x, 3, 1, 1, 1, hi, wi, mutant=mutant)
    return _fields(tap, 8, mutant)


# ---- pooling operands ------------------------------------------------------------------------------------------------------------

POSITIVE = np.arange(1, 7) / 8.0                       # j / 8, j = 1 ... 6
POSITIVE_W = np.array([1, 1, 1, 1, 2, 6]) / 12.0       # skewed to the top: two positive cells of a window tie 3 times in 10
NONPOSITIVE = np.array([0.0, -0.0, -0.125, -0.5, -3.0])
NONPOSITIVE_W = np.array([0.35, 0.2, 0.2, 0.15, 0.1])
SEED = 0
# two tensors are too small for chance (4 and 16 values): theirs are written out, [h][w][c].  One cell: a positive value, both
# zeros, a negative one.  2x2 under a 3x3 window (every window holds all four cells): channel 0 ties (0, 1) with (1, 0), which
# kh-major and kw-major scans and first and last maximum order differently; channel 1 has a zero maximum next to the other
# zero; channel 2 a unique positive maximum; channel 3 negative values only, tied.
WRITTEN_OUT = {
    (1, 1, 1, 4): [[[0.75, 0.0, -0.125, -0.0]]],
    (1, 2, 2, 4): [[[0.25, -0.5, 0.5, -3.0], [0.75, 0.0, -0.125, -0.5]],
                   [[0.75, -0.0, 0.0, -0.5], [0.5, -3.0, 0.125, -3.0]]],
}


def same_case(b, hi, wi, c, k, stride):
    (ph, ho), (pw, wo) = same_pad(hi, k, stride), same_pad(wi, k, stride)
    return (b, hi, wi, c, k, stride, ph, pw, ho, wo)


# (b, hi, wi, c, k, stride, pad_h, pad_w, ho, wo)
POOL2_CASES = [same_case(*s, 2, 2) for s in ((2, 8, 6, 8), (1, 7, 5, 12), (2, 9, 1, 8), (2, 1, 9, 8), (1, 1, 1, 4), (3, 37, 38, 136))]
POOL3_CASES = [same_case(*s, 3, 1) for s in ((2, 5, 7, 8), (1, 1, 1, 4), (1, 2, 2, 4), (1, 1, 6, 12), (2, 19, 19, 128),
                                             (1, 129, 129, 512))]
FALLBACK_CASES = [same_case(2, 10, 7, 8, 3, 2), same_case(1, 6, 5, 8, 2, 1), same_case(1, 11, 9, 4, 5, 3),
                  (1, 6, 6, 8, 2, 2, 1, 1, 4, 4)]


def case_id(case):
    b, hi, wi, c, k, stride, pad_h, pad_w, ho, wo = case
    return f'{b}x{hi}x{wi}x{c} k{k} s{stride} pad{pad_h},{pad_w}'


def p_positive(case):
    """the share of positive cells: a window of n cells has no positive cell with probability (1 - p)^n, which is set to 0.08
    for the mean n of the case's windows (cells outside the image do not count), and p is at most 0.6: windows of 4 cells need
    more positive cells than windows of 9 or 25 for the three kinds of window (tied positive maximum, no positive cell, unique
    positive maximum) to be all common"""
    b, hi, wi, c, k, stride, pad_h, pad_w, ho, wo = case
    rows = np.mean([sum(0 <= o * stride - pad_h + kk < hi for kk in range(k)) for o in range(ho)])
    cols = np.mean([sum(0 <= o * stride - pad_w + kk < wi for kk in range(k)) for o in range(wo)])
    return min(0.6, 1 - 0.08 ** (1 / (rows * cols)))


def integers(shape, mul, off):
    """integers -12 ... 12, asymmetric in every index"""
    B, H, W, C = np.meshgrid(*[np.arange(s) for s in shape], indexing='ij')
    i = mul[0] * B + mul[1] * H + mul[2] * W + mul[3] * C + (H * W) % 5 + (B * C) % 3 + (H * C) % 7 + (W * (C // 4)) % 2 + off
    return (i % 25 - 12).astype(np.float64)


class Operands:
    pass


def operands(case, dtype='fp32'):
    """case = (b, hi, wi, c, k, stride, pad_h, pad_w, ho, wo).  x from a small set of bf16 values (zeros of both signs,
    negatives, j / 8), dy and prev integers of at most 12: a sum of up to 9 gradients and prev is an integer below 256, exact in
    fp32 and a bf16 value, so the expectation holds value for value in both types (dtype only names the storage; the values are
    the same)."""
    assert dtype in ('fp32', 'bf16')
    b, hi, wi, c, k, stride, pad_h, pad_w, ho, wo = case
    rng = np.random.default_rng(zlib.crc32(repr(tuple(case)).encode()) + SEED)
    p = p_positive(case)
    n = b * hi * wi * c
    pos = rng.choice(POSITIVE, n, p=POSITIVE_W)
    non = rng.choice(len(NONPOSITIVE), n, p=NONPOSITIVE_W)
    o = Operands()
    o.case, o.dtype = tuple(case), dtype
    o.x = np.where(rng.random(n) < p, pos, NONPOSITIVE[non]).reshape(b, hi, wi, c)
    if (b, hi, wi, c) in WRITTEN_OUT:
        o.x = np.array(WRITTEN_OUT[(b, hi, wi, c)]).reshape(b, hi, wi, c)
    o.dy = integers((b, ho, wo, c), (3, 5, 7, 11), 1)
    o.prev = integers((b, hi, wi, c), (7, 3, 11, 5), 4)
    assert np.abs(o.dy).max() <= 12 and np.abs(o.prev).max() <= 12 and (k // stride + (k % stride > 0)) ** 2 <= 9
    return o


def expectation(o, mutant=None):
    """everything the entry points produce for the operands: {name: array}"""
    b, hi, wi, c, k, stride, pad_h, pad_w, ho, wo = o.case
    e = {}
    y, tap, g = gather(o.x, k, stride, pad_h, pad_w, ho, wo, o.dy, mutant)
    for acc in (0, 1):
        for mask in (0, 1):
            e[f'dx acc={acc} mask={mask}'] = finish_dx(g, o.x, o.prev, acc, mask, mutant)
    e['y'] = y
    if (k, stride, pad_h, pad_w) == (2, 2, 0, 0):
        e['rec'] = record_2x2(o.x, mutant)
        for mask in (0, 1):
            e[f'rec dx mask={mask}'] = rec_bwd(e['rec'], o.dy, mask, hi, wi)
    if (k, stride, pad_h, pad_w) == (3, 1, 1, 1):
        e['arg'] = arg_3x3(o.x, mutant)
    return e


def window_kinds(o):
    """shares of (window, channel) pairs: (positive maximum in two or more cells, no positive cell, unique positive maximum)"""
    b, hi, wi, c, k, stride, pad_h, pad_w, ho, wo = o.case
    y, _, _ = maxpool(o.x, k, stride, pad_h, pad_w, ho, wo)
    hits = np.zeros(y.shape, int)
    for _, kh, kw in _taps(k, None):
        hh, vh = _window_rows(ho, stride, pad_h, kh, hi)
        ww, vw = _window_rows(wo, stride, pad_w, kw, wi)
        if vh.any() and vw.any():
            sel = np.ix_(np.arange(b), np.flatnonzero(vh), np.flatnonzero(vw), np.arange(c))
            hits[sel] += o.x[:, hh[vh]][:, :, ww[vw]] == y[sel]
    return float(((y > 0) & (hits >= 2)).mean()), float((y <= 0).mean()), float(((y > 0) & (hits == 1)).mean())


# ---- bf16 ------------------------------------------------------------------------------------------------------------------------

def bf16_round(a):
    """fp32 values -> nearest bf16, ties to even, as float64"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def bf16_half_ulp(a):
    """half the spacing of the bf16 grid at magnitude a (8 significant bits); 0 at 0"""
    a = np.abs(np.asarray(a, np.float64))
    e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    return np.where(a > 0, 2.0 ** (e - 8), 0.0)


# ---- L2 norm -----------------------------------------------------------------------------------------------------------------------

def chunks(C):
    """J of the kernel instance that runs C channels (1, 2, or 4 for anything above 512)"""
    j = (C + 255) // 256
    return j if j <= 2 else 4


def k_fwd(J):
    return 2 * J + 8


def k_bwd(J):
    return 10 * J + 30


def l2_blocks(npix):
    return min(512, max(1, (npix + 3) // 4))


def wave_pixels(npix, J):
    """[waves][n] pixel numbers in the order a wave of l2norm_bwd_kernel adds them to its dscale partial (-1 = none)"""
    nwaves, px = 4 * l2_blocks(npix), (4 if J <= 2 else 2)
    rows = []
    for w in range(nwaves):
        rows.append([p0 + q for p0 in range(w * px, npix, nwaves * px) for q in range(px) if p0 + q < npix])
    n = max(len(r) for r in rows)
    return np.array([r + [-1] * (n - len(r)) for r in rows], int).reshape(nwaves, n)


def colsum_groups(nrows):
    """colsum_kernel: for each of the 16 row groups the rows of its four running sums, in order"""
    out = []
    for rg in range(16):
        s = [[], [], [], []]
        r = rg
        while r + 48 < nrows:
            for i in range(4):
                s[i].append(r + 16 * i)
            r += 64
        while r < nrows:
            s[0].append(r)
            r += 16
        out.append(s)
    return out


def chain_length(npix, J):
    """the longest chain of additions a term of dscale goes through: the lane's loop over its pixels, (w0 + w1) + (w2 + w3) of
    the workgroup, the longest running sum of colsum_kernel, its (s0 + s1) + (s2 + s3), and the 16 row groups one after another"""
    lane = wave_pixels(npix, J).shape[1]
    rows = max(len(s) for grp in colsum_groups(l2_blocks(npix)) for s in grp)
    return lane + 2 + rows + 2 + 16


def l2norm(x, scale, dy, eps=EPS):
    """x, dy [npix][C], scale [C] -> dict: y, dx, dscale (float64) and the bound terms y_abs = |y|, dx_abs = |scale g r| +
    |x| r^3 sum_c |scale g x|, ds_abs = sum_pix |g x r|"""
    x, scale, g = np.asarray(x, np.float64), np.asarray(scale, np.float64), np.asarray(dy, np.float64)
    ss = (x * x).sum(1, keepdims=True)
    r = 1.0 / np.sqrt(np.maximum(ss, eps))
    t = (scale * g * x).sum(1, keepdims=True)
    k = np.where(ss > eps, t * r ** 3, 0.0)
    T = np.abs(scale * g * x).sum(1, keepdims=True)
    return dict(y=scale * x * r, dx=scale * g * r - x * k, dscale=(g * x * r).sum(0),
                y_abs=np.abs(scale * x * r), dx_abs=np.abs(scale * g * r) + np.abs(x) * r ** 3 * T, ds_abs=np.abs(g * x * r).sum(0))


def l2_bounds(ref, npix, C, bf16=False):
    """-> (bound of y, of dx, of dscale), per element"""
    J = chunks(C)
    by, bdx = k_fwd(J) * U * ref['y_abs'], k_bwd(J) * U * ref['dx_abs']
    bds = (chain_length(npix, J) + k_fwd(J)) * 2.0 ** -23 * ref['ds_abs']
    if bf16:
        by, bdx = by + bf16_half_ulp(ref['y']), bdx + bf16_half_ulp(ref['dx'])
    return by, bdx, bds


L2_CASES = [(1, 4), (3, 4), (6, 64), (5, 256), (8, 256), (9, 252), (9, 260), (17, 516), (7, 1000), (130, 1024), (77, 512), (2888, 512)]


def l2_operands(npix, C, bf16=False):
    """x of both signs, scale around 20, dy; the last pixel holds a single 2^-21 (its sum of squares is below the clamp with a
    nonzero x), the one before it is all zero, the one before that holds a single 2^-19 (just above the clamp).  bf16: x and dy
    are rounded to bf16 values first."""
    rng = np.random.default_rng(1000 * npix + C)
    x = rng.normal(0, 1, (npix, C)).astype(np.float32)
    scale = (20 + rng.normal(0, 1, (C,))).astype(np.float32)
    dy = rng.normal(0, 1, (npix, C)).astype(np.float32)
    special = {}
    for name, pix, v in (('below', npix - 1, 2.0 ** -21), ('zero', npix - 2, 0.0), ('above', npix - 3, 2.0 ** -19)):
        if pix >= 0:
            x[pix] = 0
            x[pix, C // 2] = v
            special[name] = pix
    if bf16:
        x, dy = bf16_round(x).astype(np.float32), bf16_round(dy).astype(np.float32)
    return x, scale, dy, special


def _f32_lane_sums(terms, C, J, grouped):
    """terms [npix][C] fp32 -> [npix] fp32 sums in the kernels' order: a lane adds its chunks (grouped: ((a + b) + c) + d of a
    chunk first, as l2norm_fwd_kernel does; else one term after the other), then six xor-shuffle levels"""
    npix = terms.shape[0]
    pad = np.zeros((npix, 256 * J), np.float32)
    pad[:, :C] = terms
    t = pad.reshape(npix, J, 64, 4)
    s = np.zeros((npix, 64), np.float32)
    for j in range(J):
        if grouped:
            s = s + (((t[:, j, :, 0] + t[:, j, :, 1]) + t[:, j, :, 2]) + t[:, j, :, 3])
        else:
            for e in range(4):
                s = s + t[:, j, :, e]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lanes ^ o]
    assert s.dtype == np.float32 and (s == s[:, :1]).all()
    return s[:, 0]


def l2norm_f32_emulation(x, scale, dy):
    """fp32 numpy in the summation order of l2norm_fwd_kernel / l2norm_bwd_kernel / colsum_kernel (no fma; 1 / sqrt for rsqrtf):
    a check of the derivation of the bounds, not of the kernels.  -> y, dx, dscale (fp32)"""
    x, scale, g = np.asarray(x, np.float32), np.asarray(scale, np.float32), np.asarray(dy, np.float32)
    npix, C = x.shape
    J = chunks(C)
    one, eps = np.float32(1), np.float32(1e-12)
    ss = _f32_lane_sums(x * x, C, J, True)
    y = scale * x * (one / np.sqrt(np.maximum(ss, eps)))[:, None]
    ss = _f32_lane_sums(x * x, C, J, False)
    t = _f32_lane_sums(scale * g * x, C, J, False)
    r = one / np.sqrt(np.maximum(ss, eps))
    k = np.where(ss > eps, t * r * r * r, np.float32(0))
    dx = scale * g * r[:, None] - x * k[:, None]
    term = g * x * r[:, None]
    order = wave_pixels(npix, J)
    ds = np.zeros((order.shape[0], C), np.float32)
    for i in range(order.shape[1]):
        ds = ds + np.where(order[:, i:i + 1] >= 0, term[np.maximum(order[:, i], 0)], np.float32(0))
    ds = ds.reshape(-1, 4, C)
    ws = (ds[:, 0] + ds[:, 1]) + (ds[:, 2] + ds[:, 3])
    tot = np.zeros(C, np.float32)
    for grp in colsum_groups(ws.shape[0]):
        s = [np.zeros(C, np.float32) for _ in range(4)]
        for i in range(4):
            for row in grp[i]:
                s[i] = s[i] + ws[row]
        tot = tot + ((s[0] + s[1]) + (s[2] + s[3]))
    assert y.dtype == dx.dtype == tot.dtype == np.float32
    return y, dx, tot
