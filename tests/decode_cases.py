"""Crafted inputs for the argmax decode + per-class NMS (ssd_decode_nms / ssd_decode_nms_dev: detect_scan_kernel,
detect_scan_wide_kernel, detect_image_kernel<32|128>, nms_segment) and for ssd_nms_boxes (nms_boxes_kernel), with their
oracle results.  Pure numpy: tests/test_decode_cases.py proves on the CPU that every case reaches the edge it names,
tests/test_gpu_decode_edges.py runs the cases on the GPU.

A case is ONE image: pred [1, A, C+5] f32 with the call's parameters (thr, cap, max_out, out_cap, nms; cap / max_out None =
no limit, the C ABI's -1) and `edge`, a dict that names what the image is built to hit.  Class columns stay inside the
contract: finite, non-negative, no -0.0 (rows need not sum to 1).  `batches()` stacks the images that share call parameters.

Which (preset, C) gets which family -- the anchor count is the preset's, so the cost of a case is the oracle's Python loop
over its candidates, and the table spends it where the code branches:
  vgg300 C=20   every family (narrow scan, NCLS = 32, 35 scan segments: the one-wave prefix)
  vgg300 C=1    counts (small set), argmax background rows, ties         (nfg = 1: the argmax loop does not run)
  vgg300 C=27   counts (small set), argmax, ties                         (nv = 32 = SCAN_MAXV, the widest narrow row)
  vgg300 C=28   counts (small set), argmax with 4 lanes per row, ties, the threshold (the narrowest wide row, NCLS = 128)
  vgg300 C=127  counts (small set), argmax with both classes >= 28, ties (the widest row)
  vgg512 C=20   counts {0, 1025, 2049, 4097, A}, ties, caps on n = A     (96 scan segments: the serial prefix, A2 = 32768)
  vgg512 C=28   counts {0, A}, ties                                      (wide scan over 96 segments)
The per-family parameter families (caps, max_out, thresholds, segments, IoU on the line, box arithmetic) do not depend on
the row width or the preset beyond what the above covers, and run at vgg300 C=20 only."""
import functools

import numpy as np

from oracle import boxes as ob

F32 = np.float32
A_OF = {'vgg300': 8732, 'vgg512': 24564}
COMBOS = [('vgg300', 20), ('vgg300', 1), ('vgg300', 27), ('vgg300', 28), ('vgg300', 127), ('vgg512', 20), ('vgg512', 28)]
THR = 0.5                     # the default threshold of the cases that are not about the threshold
COUNTS = (0, 1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 4096, 4097, 'A')
SEG_LENGTHS = (31, 32, 33, 34, 63, 64, 65, 1100)      # (34: the first length at which pivot 32 has a box behind it)
CHAIN_BREAKS = (0, 31, 40, 63)          # links k -> k+1 taken out of the second chain (see _chain_boxes)


@functools.lru_cache(maxsize=None)
def anchors(pname):
    return ob.anchors(ob.get_preset(pname))


class Case:
    def __init__(self, name, pname, C, pred, edge, thr=THR, cap=None, max_out=None, out_cap=None, nms=1):
        A = A_OF[pname]
        assert pred.shape == (A, C + 5) and pred.dtype == F32
        fg = pred[:, :C + 1]
        assert np.isfinite(fg).all() and (fg >= 0).all() and not np.signbit(fg).any(), name      # the contract
        pred.setflags(write=False)
        self.name, self.pname, self.C, self.pred, self.edge = name, pname, C, pred, edge
        self.thr = float(F32(thr))
        self.cap, self.max_out, self.nms = cap, max_out, int(nms)
        self.out_cap = A if out_cap is None else int(out_cap)

    @property
    def params(self):
        """what one library call fixes for all its images"""
        return (self.pname, self.C, self.thr, self.cap, self.max_out, self.out_cap, self.nms)

    def __repr__(self):
        return 'Case(%s)' % self.name


# ---------------------------------------------------------------------------------------------------------------------
# building blocks
# ---------------------------------------------------------------------------------------------------------------------
def _quiet(pname, C, seed):
    """rows that are no candidate at any threshold used here above 0: foreground values 0, background 1, small offsets"""
    A = A_OF[pname]
    rng = np.random.default_rng(seed)
    pred = np.zeros((A, C + 5), F32)
    pred[:, C] = 1
    pred[:, C + 1:] = rng.normal(0, 0.3, (A, 4)).astype(F32)
    return pred, rng


def _noise(pred, C, rng, hi):
    """foreground values in [0, hi): below the threshold, so the comparison with it decides (and the argmax is not 0)"""
    A = pred.shape[0]
    pred[:, :C] = rng.uniform(0, hi, (A, C)).astype(F32)


def _distinct(n, rng, lo=0.51, hi=0.99):
    """n distinct float32 values in [lo, hi] in a seeded order"""
    v = (lo + (hi - lo) * (np.arange(n, dtype=np.float64) + 0.5) / max(n, 1)).astype(F32)
    assert len(np.unique(v)) == n
    rng.shuffle(v)
    return v


def _plant(pred, C, rows, cls, conf):
    pred[rows, :C] = 0
    pred[rows, cls] = conf
    pred[rows, C] = np.maximum(F32(0), F32(1) - np.asarray(conf, F32))


def _offsets_for(pname, a, box):
    """f32 offsets that put anchor a's decoded box near the grid box (xmin, xmax, ymin, ymax); what it really decodes to is
    the oracle's business"""
    acx, acy, aw, ah = anchors(pname)[a]
    cx = (box[0] + box[1]) / 2000.0; cy = (box[2] + box[3]) / 2000.0
    w = (box[1] - box[0]) / 1000.0; h = (box[3] - box[2]) / 1000.0
    return np.array([(cx - acx) / aw * 10, (cy - acy) / ah * 10, np.log(w / aw) * 5, np.log(h / ah) * 5], F32)


# ---------------------------------------------------------------------------------------------------------------------
# family 1: candidate counts
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _counts_pred(pname, C, n):
    A = A_OF[pname]
    pred, rng = _quiet(pname, C, 100 + n + C)
    _noise(pred, C, rng, 0.45)
    rows = np.sort(rng.choice(A, n, replace=False))
    cls = rng.integers(0, C, n)
    if n >= C:
        cls[:C] = rng.permutation(C)        # every class present
    _plant(pred, C, rows, cls, _distinct(n, rng))
    return pred


def counts(pname, C, which=COUNTS):
    out = []
    for n in which:
        nn = A_OF[pname] if n == 'A' else n
        pred = _counts_pred(pname, C, nn)
        for nms in (1, 0):
            out.append(Case('count-%s-%s' % (n, 'nms' if nms else 'dec'), pname, C, pred, dict(family='counts', n=nn), nms=nms))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# family 2 / 3: caps, max_out, out_cap
# ---------------------------------------------------------------------------------------------------------------------
CAPS = {600: (1, 599, 600, 601), 1500: (1024, 1025, 1499, 1500), 'A': (200, 2048, 2049, 5000)}


def caps(pname, C, which=(600, 1500, 'A')):
    out = []
    for n in which:
        nn = A_OF[pname] if n == 'A' else n
        pred = _counts_pred(pname, C, nn)
        for cap in CAPS[n]:
            out.append(Case('cap-%s-%d' % (n, cap), pname, C, pred, dict(family='caps', n=nn, m=min(nn, cap)), cap=cap))
            if n == 600:
                out.append(Case('cap-%s-%d-dec' % (n, cap), pname, C, pred, dict(family='caps', n=nn, m=min(nn, cap)), cap=cap, nms=0))
    if 600 in which:
        out.append(Case('cap-600-0', pname, C, _counts_pred(pname, C, 600), dict(family='caps', n=600, m=0), cap=0))
    return out


def max_outs(pname, C):
    pred = _counts_pred(pname, C, 600)
    base = Case('tmp', pname, C, pred, {})
    s = int(expected(base)['count'])
    out = []
    for mo in (0, 1, s - 1, s, s + 1):
        out.append(Case('max-out-%d' % mo, pname, C, pred, dict(family='max_out', survivors=s, count=min(s, mo)), max_out=mo))
    out.append(Case('max-out-1-dec', pname, C, pred, dict(family='max_out', survivors=600, count=1), max_out=1, nms=0))
    # out_cap below the count: count is not clipped by it, rows past it are not written
    out.append(Case('out-cap-7', pname, C, pred, dict(family='out_cap', survivors=s, count=s), out_cap=7))
    out.append(Case('out-cap-7-max-out', pname, C, pred, dict(family='out_cap', survivors=s, count=s - 1), out_cap=7, max_out=s - 1))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# family 4: ties
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ties_pred(pname, C, n):
    """n candidates (None: every anchor) with confidences k/8, k = 1..8"""
    A = A_OF[pname]
    pred, rng = _quiet(pname, C, 200 + C)
    rows = np.arange(A) if n is None else np.sort(rng.choice(A, n, replace=False))
    k = rng.integers(1, 9, len(rows))
    _plant(pred, C, rows, rng.integers(0, C, len(rows)), (k / 8.0).astype(F32))
    return pred


def ties(pname, C):
    A = A_OF[pname]
    out = [Case('ties-all', pname, C, _ties_pred(pname, C, None), dict(family='ties', n=A), thr=0.01),
           Case('ties-all-dec', pname, C, _ties_pred(pname, C, None), dict(family='ties', n=A), thr=0.01, nms=0)]
    if pname == 'vgg300':
        small = _ties_pred(pname, C, 800)
        out += [Case('ties-800', pname, C, small, dict(family='ties', n=800), thr=0.01),
                Case('ties-800-dec', pname, C, small, dict(family='ties', n=800), thr=0.01, nms=0)]
    if (pname, C) in (('vgg300', 20), ('vgg512', 20)):
        # a cap whose cut falls inside a run of equal confidences (cut_in_run() says where; the CPU test checks it)
        for n, pred, cap in ((A, _ties_pred(pname, C, None), 3000), (A, _ties_pred(pname, C, None), 1000),
                             (800, _ties_pred(pname, C, 800) if pname == 'vgg300' else None, 300)):
            if pred is not None:
                out.append(Case('ties-%d-cap-%d' % (n, cap), pname, C, pred, dict(family='ties-cap', n=n, cap=cap), thr=0.01, cap=cap))
    if C >= 6:
        # two classes share the best confidence: the class of the lower anchor leads the groups
        pred, rng = _quiet(pname, C, 210 + C)
        rows = np.array([100, 200, 300, 400, 5000, 5001, 7000])
        cls = np.array([5, 3, 5, 3, 1, 3, 5])
        conf = np.array([0.9, 0.9, 0.75, 0.8, 0.9, 0.6, 0.6], F32)
        _plant(pred, C, rows, cls, conf)
        edge = dict(family='ties-class-order', group_order=[5, 3, 1])
        out += [Case('ties-class-order', pname, C, pred, edge), Case('ties-class-order-cap', pname, C, pred, edge, cap=6)]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# family 5: the threshold
# ---------------------------------------------------------------------------------------------------------------------
def thresholds(pname, C):
    A = A_OF[pname]
    out = []
    for thr in (F32(0.5), F32(0.01), F32(0.0)):
        pred, rng = _quiet(pname, C, 300 + int(thr * 100))
        below, above = np.nextafter(thr, F32(0)), np.nextafter(thr, F32(1))
        rows = np.sort(rng.choice(A, 90, replace=False))
        vals = np.tile(np.array([thr, below, above], F32), 30)
        _plant(pred, C, rows, rng.integers(0, C, 90), vals)
        far = np.setdiff1d(np.arange(A), rows)[:40]
        _plant(pred, C, far, rng.integers(0, C, 40), _distinct(40, rng, 0.6, 0.9))
        at = rows[vals == thr]
        if thr == 0:
            # below == thr == 0; `above` is the smallest subnormal, in a class other than 0 (the argmax must see it)
            pred[rows[vals == above], :C] = 0
            pred[rows[vals == above], 1 % C] = above
            n = A
        else:
            n = int(((vals >= thr).sum()) + 40)
        edge = dict(family='threshold', n=n, at=at, just_below=rows[vals == below] if thr > 0 else at[:0], just_above=rows[vals == above])
        out.append(Case('thr-%g' % thr, pname, C, pred, edge, thr=thr))
        out.append(Case('thr-%g-dec' % thr, pname, C, pred, edge, thr=thr, nms=0))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# family 6: the argmax of a row
# ---------------------------------------------------------------------------------------------------------------------
def argmax_rows(pname, C):
    """-> one case; edge['want'] = {anchor: class} for every crafted row"""
    A = A_OF[pname]
    pred, rng = _quiet(pname, C, 400 + C)
    _noise(pred, C, rng, 0.3)
    pairs = []
    if C >= 2:
        if C <= 27:
            pairs = [(0, 1), (0, C - 1), (C - 2, C - 1), (C // 2, C // 2 + 1), (1, C - 1)]
        else:
            # all sixteen (c1 mod 4, c2 mod 4) combinations, the lower class first and second in lane order
            for r1 in range(4):
                for r2 in range(4):
                    c1 = 4 + r1
                    c2 = 8 + r2 + (4 if r1 == r2 else 0)
                    pairs.append((c1, c2))
                    pairs.append((c1 + 12, c2 + 8))                      # further up, below 28
                    if C > 60:
                        pairs.append((28 + c1, 60 + c2))                 # both classes >= 28
            pairs += [(0, C - 1), (C - 2, C - 1), (3, C - 1), (C - 5, C - 1)]
        pairs = sorted({(min(a, b), max(a, b)) for a, b in pairs if a != b and max(a, b) < C})
    want = {}
    row = 37                                   # rows spread over several scan blocks, and over the 4 row lanes of a wide chunk
    for c1, c2 in pairs:
        pred[row, :C] = rng.uniform(0, 0.3, C).astype(F32)
        pred[row, c1] = pred[row, c2] = F32(0.75)
        want[row] = c1
        row += 53
        pred[row, :C] = rng.uniform(0, 0.3, C).astype(F32)            # three equal maxima
        pred[row, c1] = pred[row, c2] = pred[row, (c1 + c2) // 2] = F32(0.625)
        want[row] = c1
        row += 53
    for c in sorted({C - 1, max(C - 2, 0), max(C - 3, 0), max(C - 4, 0), 0}):     # a lone maximum in the last classes
        pred[row, :C] = rng.uniform(0, 0.3, C).astype(F32)
        pred[row, c] = F32(0.875)
        want[row] = c
        row += 53
    bg = {}
    for k, (c, fgv, bgv) in enumerate([(C - 1, 0.7, 0.95), (0, 0.7, 0.7), (C // 2, 0.55, 1.0), (C - 1, 0.6, 0.6)]):
        pred[row, :C] = rng.uniform(0, 0.3, C).astype(F32)
        pred[row, c] = F32(fgv)
        pred[row, C] = F32(bgv)               # background above / equal to the best foreground: still a candidate
        want[row] = c
        bg[row] = c
        row += 53
    # background large, every foreground value below the threshold: not a candidate
    pred[row, :C] = F32(0.2)
    pred[row, C] = F32(0.99)
    edge = dict(family='argmax', want=want, background=bg, not_candidate=row, pairs=pairs)
    assert row < A
    return [Case('argmax', pname, C, pred, edge), Case('argmax-dec', pname, C, pred, edge, nms=0)]


# ---------------------------------------------------------------------------------------------------------------------
# family 7: class segments of chosen lengths; chains of boxes where the survivor depends on the order
# ---------------------------------------------------------------------------------------------------------------------
def _chain_boxes(L, breaks=()):
    """grid boxes of side 40 along diagonals, consecutive ones shifted by 6 (IoU about 0.57, two apart about 0.33): box k
    overlaps k+1 above 0.45 and k+2 below it.  A link k -> k+1 in `breaks` is shifted by 14 (IoU about 0.27).  100 to a row."""
    out = []
    x = y = 0
    for k in range(L):
        if k % 100 == 0:
            x, y = 10, 10 + 45 * (k // 100)
        out.append((x, x + 40, y, y + 40))
        step = 14 if k in breaks else 6
        x += step
        y += step if k // 100 == 0 and L <= 100 else 0
    return out


def chain_survivors(L, breaks=()):
    """greedy NMS on a chain whose only overlaps are the unbroken links (chains of one row: L <= 100)"""
    alive = []
    for k in range(L):
        linked = k > 0 and (k - 1) not in breaks
        alive.append(not (linked and alive[k - 1]))
    return [k for k in range(L) if alive[k]]


def segments(pname, C, lengths=SEG_LENGTHS):
    A = A_OF[pname]
    out = []
    for L in lengths:
        for breaks in ((), CHAIN_BREAKS):
            if breaks and L < 65:
                continue
            pred, rng = _quiet(pname, C, 500 + L)
            chain_cls = 7 % C
            # the chain sits on consecutive anchors near the end of the table; confidence falls along the chain
            rows = np.arange(A - 1200, A - 1200 + L)
            conf = (0.9 - 0.35 * np.arange(L) / max(L, 1)).astype(F32)
            _plant(pred, C, rows, chain_cls, conf)
            for k, bx in enumerate(_chain_boxes(L, breaks)):
                pred[rows[k], C + 1:] = _offsets_for(pname, rows[k], bx)
            # other classes of mixed length around it; one of them holds the best confidence, so the chain is not segment 0
            others = {}
            free = rng.permutation(A - 1300)
            used = 0
            for c, ln in ((2 % C, 5), (11 % C, 40), (0, 70), (15 % C, 17), (4 % C, 33)):
                if c == chain_cls or c in others:
                    continue
                r = np.sort(free[used:used + ln]); used += ln
                _plant(pred, C, r, c, _distinct(ln, rng, 0.55, 0.99 if c == 2 % C else 0.9))
                others[c] = ln
            edge = dict(family='segments', chain_cls=chain_cls, L=L, breaks=breaks, others=others, chain_rows=rows,
                        n=L + sum(others.values()))
            out.append(Case('segment-%d%s' % (L, '-broken' if breaks else ''), pname, C, pred, edge))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# family 8: IoU on the line, 20 inter - 9 union = 0 / small positive / small negative
# ---------------------------------------------------------------------------------------------------------------------
# (first anchor, second anchor, offsets of the first, offsets of the second, 20 inter - 9 union) found by search_iou_line()
_IOU_LINE_FOUND = (
    (8726, 8727, [-1.0764968395233154, 0.3199852705001831, 0.2203536331653595, 0.45221179723739624],
     [-0.5651858448982239, -0.6392504572868347, -0.033403802663087845, -0.5186586380004883], 0),      # inter 262350, union 583000
    (8728, 8729, [0.3445107638835907, 0.5614568591117859, -1.1917855739593506, 0.2751286029815674],
     [-0.4265855848789215, -0.022699685767292976, 0.5579307675361633, -1.1175261735916138], 150),     # inter 362100, union 804650
    (8730, 8731, [-0.06168224290013313, -0.5067574381828308, -1.4402656555175781, -0.7169786095619202],
     [-0.695747435092926, 0.0067902724258601665, 0.3551937937736511, -0.9553585052490234], -588),     # inter 388614, union 863652
)


def pair_boxes(pname, a, la, b, lb):
    """the round-tripped integer boxes NMS compares for two (anchor, offsets) rows, and (inter, union, 20 inter - 9 union)"""
    an = anchors(pname)
    bx = []
    for i, l in ((a, la), (b, lb)):
        l = np.minimum(np.asarray(l, F32), F32(100))
        bx.append(ob.normalize_abs_np2(*ob.decode_location_np2(l, an[i])))
    r = ob.nms_roundtrip(np.array(bx, np.int64))
    w = max(0, min(r[0, 1], r[1, 1]) - max(r[0, 0], r[1, 0]) + 1)
    h = max(0, min(r[0, 3], r[1, 3]) - max(r[0, 2], r[1, 2]) + 1)
    inter = int(w * h)
    union = int((r[0, 1] - r[0, 0] + 1) * (r[0, 3] - r[0, 2] + 1) + (r[1, 1] - r[1, 0] + 1) * (r[1, 3] - r[1, 2] + 1) - inter)
    return r, inter, union, 20 * inter - 9 * union


def search_iou_line(pname='vgg300', draws=900000, seed=5):
    """How _IOU_LINE_FOUND was found (not called by any test): seeded random offsets on the preset's last anchors, keeping per
    anchor pair the draw with 20 inter - 9 union == 0, the smallest positive and the largest negative value.  (A minute of
    CPU; one pair of anchors serves one sign, so the table takes 0 from the first pair, +150 from the second and -588 from the
    third: against 20 inter of about 7.5 million these are within 1e-4 of the line.)"""
    A = A_OF[pname]
    rng = np.random.default_rng(seed)
    best = {}
    pairs = [(A - 2, A - 1), (A - 4, A - 3), (A - 6, A - 5)]
    for t in range(draws):
        a, b = pairs[t % 3]
        la = rng.normal(0, 0.5, 4).astype(F32); lb = rng.normal(0, 0.5, 4).astype(F32)
        _, inter, union, d = pair_boxes(pname, a, la, b, lb)
        if inter == 0:
            continue
        kind = 'zero' if d == 0 else ('pos' if d > 0 else 'neg')
        key = (kind, (a, b))
        if key not in best or abs(d) < abs(best[key][4]):
            best[key] = (a, b, [float(v) for v in la], [float(v) for v in lb], d, inter, union)
    return best


def iou_line(pname, C):
    """the three pairs in three classes of one image; edge['pairs'] = [(first row, second row, 20 inter - 9 union)]"""
    assert pname == 'vgg300' and C >= 3
    pred, rng = _quiet(pname, C, 600)
    pairs = []
    for c, (a, b, la, lb, d) in enumerate(_IOU_LINE_FOUND):
        _plant(pred, C, np.array([a, b]), c, np.array([0.9 - 0.1 * c, 0.8 - 0.1 * c], F32))
        pred[a, C + 1:] = np.array(la, F32)
        pred[b, C + 1:] = np.array(lb, F32)
        pairs.append((a, b, d))
    return [Case('iou-line', pname, C, pred, dict(family='iou-line', pairs=pairs))]


# ---------------------------------------------------------------------------------------------------------------------
# family 9: box arithmetic
# ---------------------------------------------------------------------------------------------------------------------
def nonfinite_rows(pred, C):
    """rows whose decoded box is not finite: NaN in any offset (NaN > 100 is false: it passes the clamp), -inf in a centre
    offset.  +inf clamps to 100; -inf in a size offset gives the finite size 0."""
    loc = pred[:, C + 1:]
    return np.isnan(loc).any(1) | np.isneginf(loc[:, :2]).any(1)


def box_arith(pname, C):
    A = A_OF[pname]
    an = anchors(pname)
    pred, rng = _quiet(pname, C, 700)
    cls = 2 % C
    # anchors on which a centre offset of 100 stays inside the grid (small, near the origin): there 99, 99.5 and 100 differ
    ax = np.argsort(an[:, 0] + 10 * an[:, 2])[:12]
    ay = np.argsort(an[:, 1] + 10 * an[:, 3])[:12]
    big = [F32(100), np.nextafter(F32(100), F32(np.inf)), F32(1e9), F32(np.inf)]
    rows, kinds = [], {}
    free = iter([int(r) for r in rng.permutation(np.setdiff1d(np.arange(A - 40), np.concatenate([ax, ay])))])

    def put(row, slot, v, kind, conf):
        pred[row, C + 1:] = F32(0.1)
        pred[row, C + 1 + slot] = v
        rows.append(row); kinds[row] = (kind, slot)
        _plant(pred, C, np.array([row]), cls, F32(conf))

    conf = iter(_distinct(200, rng, 0.55, 0.98))
    for slot in range(4):
        for j, v in enumerate(big + [F32(99.5), np.nextafter(F32(99), F32(np.inf)), np.nextafter(F32(100), F32(0))]):
            row = int(ax[j]) if slot == 0 else int(ay[j]) if slot == 1 else next(free)
            put(row, slot, v, 'clamp', next(conf))
    for slot in (2, 3):
        put(next(free), slot, F32(-np.inf), 'size-zero', next(conf))
        put(next(free), slot, F32(-50), 'size-tiny', next(conf))
    large = iter(range(A - 40, A))            # anchors wider than 0.3: a clamped centre offset of 100 puts the box beyond the grid
    for slot in (0, 1):
        for v in (F32(1e4), F32(-1e4), F32(40), F32(-40)):
            put(next(large), slot, v, 'outside', next(conf))
    for slot in range(4):
        put(next(free), slot, F32(np.nan), 'nan', next(conf))
        put(next(free), slot, F32(np.nan), 'nan', next(conf))       # twice: the corner boxes meet in NMS
    for slot in (0, 1):
        put(next(free), slot, F32(-np.inf), 'centre-neg-inf', next(conf))
    # one more class holding a corner box and an ordinary one
    other = 5 % C
    if other != cls:
        r = next(free)
        pred[r, C + 1:] = F32(np.nan)
        _plant(pred, C, np.array([r, next(free)]), other, np.array([0.7, 0.6], F32))
        kinds[r] = ('nan', -1)
    assert len(set(rows)) == len(rows)
    edge = dict(family='box-arith', kinds=kinds, nonfinite=np.nonzero(nonfinite_rows(pred, C))[0])
    return [Case('box-arith', pname, C, pred, edge), Case('box-arith-dec', pname, C, pred, edge, nms=0)]


# ---------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cases(pname, C):
    """every single-image case of one (preset, class count), in a fixed order"""
    if (pname, C) == ('vgg300', 20):
        out = (counts(pname, C) + caps(pname, C) + max_outs(pname, C) + ties(pname, C) + thresholds(pname, C) + argmax_rows(pname, C)
               + segments(pname, C) + iou_line(pname, C) + box_arith(pname, C))
    elif pname == 'vgg300':
        out = counts(pname, C, (0, 1, 1024, 1025, 2049, 'A')) + ties(pname, C) + argmax_rows(pname, C)
        if C == 28:
            out += thresholds(pname, C)          # the wide scan has its own comparison with the threshold
        if C in (1, 127):
            out += segments(pname, C, (33, 65)) if C > 1 else segments(pname, C, (64,))
    elif C == 20:
        out = counts(pname, C, (0, 1025, 2049, 4097, 'A')) + ties(pname, C) + caps(pname, C, ('A',)) + argmax_rows(pname, C)
    else:
        out = counts(pname, C, (0, 'A')) + ties(pname, C) + argmax_rows(pname, C)
    names = [c.name for c in out]
    assert len(set(names)) == len(names), names
    return tuple(out)


def all_cases():
    return [c for pname, C in COMBOS for c in cases(pname, C)]


def batches(pname, C):
    """family 10: the cases of one (preset, C) grouped by call parameters, each group's images in a seeded shuffle; in the
    largest group an image without candidates stands between two in which every anchor is one.  A is no multiple of the
    scan block (A mod 256 = 28 / 244), so every block that straddles two images sees unequal neighbours.
    -> [(params, [case, ...])]"""
    groups = {}
    for c in cases(pname, C):
        groups.setdefault(c.params, []).append(c)
    out = []
    for gi, (params, group) in enumerate(groups.items()):
        rng = np.random.default_rng(900 + gi)
        group = [group[i] for i in rng.permutation(len(group))]
        if params == (pname, C, float(F32(THR)), None, None, A_OF[pname], 1):
            full = next(c for c in group if c.name == 'count-A-nms')
            empty = next(c for c in group if c.name == 'count-0-nms')
            rest = [c for c in group if c is not full and c is not empty]
            group = rest[:len(rest) // 2] + [full, empty, full] + rest[len(rest) // 2:]
        out.append((params, group))
    return out


def stack(group):
    return np.ascontiguousarray(np.stack([c.pred for c in group]))


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's results
# ---------------------------------------------------------------------------------------------------------------------
_DECODED = {}


def decoded(case):
    """ob.decode of the image with no cap (every candidate, confidence descending, ties by lower anchor), shared by the cases
    that differ only in cap / max_out / nms.

    ob.decode raises on offsets whose box is not finite, as the reference does.  The LIBRARY documents a deviation there
    (decode_box, include/ssdvgg_hip.h): such a row's box is the empty corner box [0, 0, 0, 0].  So the oracle runs on a copy
    with those rows' offsets zeroed, and [0, 0, 0, 0] is then written for them: the library's behaviour, not the reference's."""
    key = (id(case.pred), case.thr)
    if key not in _DECODED:
        pred = case.pred
        bad = nonfinite_rows(pred, case.C)
        if bad.any():
            pred = pred.copy()
            pred[bad, case.C + 1:] = 0
        det = ob.decode(pred, anchors(case.pname), case.thr, None)
        det['box'][bad[det['idx']]] = 0
        for v in det.values():
            v.setflags(write=False)
        _DECODED[key] = (case.pred, det)          # (the array is kept alive: its id is the key)
    return _DECODED[key][1]


def expected(case):
    """-> dict(count, idx, cls, conf, box): what the library must write for this image (count unclipped by out_cap, the arrays
    all `count` rows).  ob.decode's list cut at cap, then ob.suppress (nms = 1) or the list itself (nms = 0), cut at max_out."""
    det = decoded(case)
    if case.cap is not None:
        det = {k: v[:case.cap] for k, v in det.items()}
    if case.nms:
        keep = ob.suppress(det, case.max_out)
    else:
        keep = np.arange(len(det['idx']))[:case.max_out]
    out = {k: v[keep] for k, v in det.items()}
    out['count'] = len(keep)
    return out


def cut_in_run(case):
    """(confidence at position cap - 1, at position cap) of the uncapped list: equal when the cap cuts a run of ties"""
    det = decoded(case)
    return det['conf'][case.cap - 1], det['conf'][case.cap]


# ---------------------------------------------------------------------------------------------------------------------
# ssd_nms_boxes: (name, boxes int32 [n,4] (xmin, xmax, ymin, ymax), conf f32 [n], group int32 [n] or None, thr, edge)
# ---------------------------------------------------------------------------------------------------------------------
def _ratio_pair(p, q, k, more=0):
    """two one-row boxes with intersection p k + more and union q k"""
    s = (q - p) * k // 2
    return [(0, s + p * k - 1, 0, 0), (s - more, q * k - 1, 0, 0)]


def _random_boxes(rng, n, lo=0, hi=900, size=(20, 300)):
    x0 = rng.integers(lo, hi, n); y0 = rng.integers(lo, hi, n)
    return np.stack([x0, x0 + rng.integers(size[0], size[1], n), y0, y0 + rng.integers(size[0], size[1], n)], 1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def nms_cases():
    out = []

    def add(name, boxes, conf, group, thr, **edge):
        boxes = np.ascontiguousarray(boxes, np.int32).reshape(-1, 4)
        conf = np.ascontiguousarray(conf, F32)
        group = None if group is None else np.ascontiguousarray(group, np.int32)
        out.append((name, boxes, conf, group, float(thr), edge))

    far = [(0, 50, 0, 50), (200, 250, 0, 50), (400, 450, 0, 50), (600, 650, 0, 50), (0, 50, 200, 250), (200, 250, 200, 250)]
    # signed zeros: equal by value, so the earlier box goes first whichever sign it carries
    add('zeros-neg-first', far[:2], [-0.0, 0.0], None, 0.45, order=[0, 1])
    add('zeros-pos-first', far[:2], [0.0, -0.0], None, 0.45, order=[0, 1])
    add('zeros-mixed', far, [-0.0, -1e-3, 0.0, 1e-3, -0.0, 0.0], None, 0.45, order=[3, 0, 2, 4, 5, 1])
    add('zeros-groups', far, [-0.0, 0.0, 0.0, -0.0, -0.0, 0.0], [0, 1, 0, 1, 0, 1], 0.45, order=[0, 2, 4, 1, 3, 5])
    add('zeros-overlap', [far[0], far[0], far[1]], [-0.0, 0.0, 0.0], None, 0.45, order=[0, 2])
    # the f64 quotient at the threshold: equality keeps the box (the comparison is >), one unit of area more drops it
    for p, q, thr in ((9, 20, 0.45), (3, 10, 0.3), (3, 5, 0.6), (1, 20, 0.05)):
        for k in (1, 40):
            add('ratio-%d-%d-k%d' % (p, q, k), _ratio_pair(p, q, k), [0.9, 0.8], None, thr, order=[0, 1], inter=p * k, union=q * k)
        add('ratio-%d-%d-more' % (p, q), _ratio_pair(p, q, 40, 1), [0.9, 0.8], None, thr, order=[0], inter=p * 40 + 1, union=q * 40)
    add('thr-0-touching', [(0, 10, 0, 10), (10, 20, 0, 10), (21, 30, 0, 10)], [0.9, 0.8, 0.7], None, 0.0, order=[0, 2])
    add('thr-1-identical', [far[0], far[0], far[0]], [0.5, 0.9, 0.7], None, 1.0, order=[1, 2, 0])
    add('one-box', [far[3]], [0.3], None, 0.45, order=[0])
    rng = np.random.default_rng(41)
    n = 4096
    add('own-groups-4096', _random_boxes(rng, n), rng.uniform(0, 1, n), rng.permutation(n), 0.45, ngroups=n)
    n = 65535
    centre = np.array([(100, 200, 100, 200), (500, 640, 300, 420), (300, 380, 700, 900)])[rng.integers(0, 3, n)]
    add('clusters-65535', centre + rng.integers(-3, 4, (n, 4)), np.round(rng.uniform(-1, 1, n) * 64) / 64, None, 0.45, n=n)
    n = 700
    add('heavy-ties', _random_boxes(rng, n, size=(40, 200)), np.round(rng.uniform(-0.5, 0.5, n) * 4) / 4 + 0.0, rng.integers(0, 5, n), 0.3,
        n=n)
    return tuple(out)


def nms_expected(boxes, conf, group, thr):
    """positions into the list in output order: ob.nms_list for one class, ob.suppress_list over groups (the group index is the
    class' first-appearance rank, which is what the C ABI takes; ob.suppress_list orders by first appearance in the list, so the
    records are passed in an order where the two agree: group g's first record before group g+1's)"""
    bx = [tuple(int(v) for v in b) for b in boxes]
    if group is None:
        return ob.nms_list([(float(c), b) for c, b in zip(conf, bx)], thr)
    order = np.argsort(group, kind='stable')
    recs = [(float(conf[i]), int(group[i]), bx[i]) for i in order]
    return [int(order[k]) for k in ob.suppress_list(recs, thr)]
