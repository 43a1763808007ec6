"""Oracle of the COCO box evaluation (include/ssdvgg_hip.h, "COCO box evaluation") in float64 numpy, written in the per-image /
accumulate structure COCO's tools use: per (image, class) sort, cap, IoU matrix and greedy matching; then per class concatenate,
stable sort, cumulative sums and searchsorted.  The kernels walk each class's detections ONCE in global confidence order with
true-positive precisions only, so the agreement of the two is a real check.  Every comparison against the kernels is ==.

Boxes are (xmin, xmax, ymin, ymax); gt_flags bit 1 (value 2) = crowd, any nonzero flag = ignored."""
import numpy as np

AREA_RANGES = ((0.0, 1e10), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10))      # all, small, medium, large
MAX_DETS = (1, 10, 100)
GROUPS = ((0, 100), (1, 100), (2, 100), (3, 100), (0, 1), (0, 10))      # (area, maxDet) of the six AR planes; the first four are AP's
REC_THRS = np.linspace(0.0, 1.0, 101)
EPS = float(np.spacing(1))                                              # 2^-52
DEFAULT_THRESHOLDS = np.linspace(0.5, 0.95, 10)
SUMMARY_NAMES = ('AP', 'AP50', 'AP75', 'APs', 'APm', 'APl', 'AR1', 'AR10', 'AR100', 'ARs', 'ARm', 'ARl')

# the mutations of tests/test_coco_ref.py: each one changes at least one hand-worked number
MUTATIONS = ('strict_threshold', 'first_on_ties', 'plus_one_iou', 'crowd_full_union', 'no_rank_cap', 'box_area_ranges')


def iou_matrix(d, g, crowd, mutate=None):
    """[n_d, n_g] float64, continuous form; against a crowd box the union is the detection's area"""
    one = 1.0 if mutate == 'plus_one_iou' else 0.0
    out = np.zeros((len(d), len(g)), np.float64)
    for i in range(len(d)):
        ad = (d[i, 1] - d[i, 0] + one) * (d[i, 3] - d[i, 2] + one)
        for j in range(len(g)):
            w = min(d[i, 1], g[j, 1]) - max(d[i, 0], g[j, 0]) + one
            h = min(d[i, 3], g[j, 3]) - max(d[i, 2], g[j, 2]) + one
            if w <= 0 or h <= 0:
                continue
            inter = w * h
            ag = (g[j, 1] - g[j, 0] + one) * (g[j, 3] - g[j, 2] + one)
            union = ad if crowd[j] and mutate != 'crowd_full_union' else (ad + ag) - inter
            out[i, j] = inter / union
    return out


def evaluate_img(ious, d_area, g_area, g_flagged, g_crowd, rng, thresholds, mutate=None):
    """One (image, class, area range): detections already sorted and capped.  Returns (dt_matched [T, D] bool, dt_ignore [T, D]
    bool, gt_ignore [G] bool)."""
    lo, hi = rng
    g_ign = g_flagged | (g_area < lo) | (g_area > hi)
    gtind = np.argsort(g_ign, kind='mergesort')                       # the non-ignored first, both parts in arrival order
    T, D, G = len(thresholds), len(d_area), len(g_area)
    gtm = np.zeros((T, G), bool)
    dtm = np.zeros((T, D), bool)
    dt_ig = np.zeros((T, D), bool)
    for tind, t in enumerate(thresholds if G else ()):
        for dind in range(D):
            best = min(float(t), 1 - 1e-10)
            m = -1
            for gind in gtind:
                if gtm[tind, gind] and not g_crowd[gind]:
                    continue
                if m > -1 and not g_ign[m] and g_ign[gind]:
                    break
                v = ious[dind, gind]
                if mutate == 'strict_threshold' and m == -1:
                    if not v > best:
                        continue
                elif mutate == 'first_on_ties' and m > -1:
                    if not v > best:
                        continue
                elif v < best:
                    continue
                best = v
                m = gind
            if m == -1:
                continue
            dt_ig[tind, dind] = g_ign[m]
            dtm[tind, dind] = True
            gtm[tind, m] = True
    outside = (d_area < lo) | (d_area > hi)
    dt_ig = dt_ig | (~dtm & outside[None, :])
    return dtm, dt_ig, g_ign


def _by_sample(idx, samples):
    """{sample: the rows of idx that belong to it, in order}"""
    order = idx[np.argsort(samples[idx], kind='mergesort')]
    s = samples[order]
    cuts = np.nonzero(np.diff(s))[0] + 1
    return {int(part_s): part for part_s, part in zip(s[np.concatenate(([0], cuts))] if len(s) else (), np.split(order, cuts))}


def evaluate(det_box, det_conf, det_cls, det_sample, gt_box, gt_cls, gt_sample, gt_flags, gt_area, sample_scale, ncls,
             thresholds=DEFAULT_THRESHOLDS, mutate=None, details=None):
    """(ap [4, T, ncls], ar [6, T, ncls], present [4, ncls] int32).  ap / ar are -1 where the class is not present under the
    area range.  details (a dict): filled with (class, group, t) -> list of 'T' / 'F' / 'I' per detection in curve order."""
    det_box = np.asarray(det_box, np.float32).reshape(-1, 4).astype(np.float64)
    det_conf = np.asarray(det_conf, np.float32); det_cls = np.asarray(det_cls, np.int64); det_sample = np.asarray(det_sample, np.int64)
    gt_box = np.asarray(gt_box, np.float64).reshape(-1, 4); gt_cls = np.asarray(gt_cls, np.int64); gt_sample = np.asarray(gt_sample, np.int64)
    gt_flags = np.asarray(gt_flags, np.int64) if gt_flags is not None else np.zeros(len(gt_cls), np.int64)
    gt_area = np.asarray(gt_area, np.float64); sample_scale = np.asarray(sample_scale, np.float64)
    thresholds = np.asarray(thresholds, np.float64)
    T = len(thresholds)
    flagged = gt_flags != 0
    crowd = (gt_flags & 2) != 0
    if mutate == 'box_area_ranges':
        gt_area = (gt_box[:, 1] - gt_box[:, 0]) * (gt_box[:, 3] - gt_box[:, 2]) * sample_scale[gt_sample] if len(gt_cls) else gt_area
    det_area = (det_box[:, 1] - det_box[:, 0]) * (det_box[:, 3] - det_box[:, 2])
    det_area = det_area * sample_scale[det_sample] if len(det_cls) else det_area
    cap_all = 10 ** 9 if mutate == 'no_rank_cap' else MAX_DETS[-1]
    ap = np.full((4, T, ncls), -1.0); ar = np.full((6, T, ncls), -1.0); present = np.zeros((4, ncls), np.int32)
    for k in range(ncls):
        dk = np.nonzero(det_cls == k)[0]
        gk = np.nonzero(gt_cls == k)[0]
        per_img = []                                                  # per image: (detections sorted and capped, ground truth, IoUs)
        d_of, g_of = _by_sample(dk, det_sample), _by_sample(gk, gt_sample)
        none = np.zeros(0, np.int64)
        for s in sorted(set(d_of) | set(g_of)):
            d, g = d_of.get(s, none), g_of.get(s, none)
            d = d[np.argsort(-det_conf[d].astype(np.float64), kind='mergesort')][:cap_all]
            per_img.append((d, g, iou_matrix(det_box[d], gt_box[g], crowd[g], mutate)))
        for a, rng in enumerate(AREA_RANGES):
            evals = [evaluate_img(ious, det_area[d], gt_area[g], flagged[g], crowd[g], rng, thresholds, mutate) for d, g, ious in per_img]
            npig = sum(int(np.count_nonzero(~e[2])) for e in evals)
            present[a, k] = npig > 0
            if npig == 0:
                continue
            for grp, (ga, max_det) in enumerate(GROUPS):
                if ga != a:
                    continue
                if mutate == 'no_rank_cap':
                    max_det = cap_all
                ids = np.concatenate([d[:max_det] for d, _, _ in per_img]) if per_img else np.zeros(0, np.int64)
                dtm = np.concatenate([e[0][:, :max_det] for e in evals], axis=1) if evals else np.zeros((T, 0), bool)
                dig = np.concatenate([e[1][:, :max_det] for e in evals], axis=1) if evals else np.zeros((T, 0), bool)
                order = np.lexsort((ids, -det_conf[ids].astype(np.float64)))      # confidence descending, arrival ascending
                dtm, dig = dtm[:, order], dig[:, order]
                tps = dtm & ~dig
                fps = ~dtm & ~dig
                tp_sum = np.cumsum(tps, axis=1).astype(np.float64)
                fp_sum = np.cumsum(fps, axis=1).astype(np.float64)
                for t in range(T):
                    tp, fp = tp_sum[t], fp_sum[t]
                    nd = len(tp)
                    rc = tp / npig
                    pr = (tp / (fp + tp + EPS)).tolist()
                    ar[grp, t, k] = rc[-1] if nd else 0.0
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    q = [0.0] * len(REC_THRS)
                    for ri, pi in enumerate(np.searchsorted(rc, REC_THRS, side='left')):
                        if pi < nd:
                            q[ri] = pr[pi]
                    if grp < 4:
                        total = 0.0
                        for v in q:
                            total = total + v
                        ap[grp, t, k] = total / 101.0
                    if details is not None:
                        details[(k, grp, t)] = ['I' if dig[t, i] else ('T' if dtm[t, i] else 'F') for i in range(nd)]
    return ap, ar, present


def _mean(x, mask):
    x = x[:, mask]
    return float(np.mean(x)) if x.size else -1.0


def summarize(ap, ar, present, thresholds=DEFAULT_THRESHOLDS):
    """The twelve numbers, in COCO's order, from one fixed expression each."""
    thresholds = np.asarray(thresholds, np.float64)
    p = present.astype(bool)

    def at(value):
        idx = np.nonzero(thresholds == value)[0]
        return _mean(ap[0][idx[:1]], p[0]) if len(idx) else -1.0
    return {'AP': _mean(ap[0], p[0]), 'AP50': at(0.5), 'AP75': at(0.75), 'APs': _mean(ap[1], p[1]), 'APm': _mean(ap[2], p[2]),
            'APl': _mean(ap[3], p[3]), 'AR1': _mean(ar[4], p[0]), 'AR10': _mean(ar[5], p[0]), 'AR100': _mean(ar[0], p[0]),
            'ARs': _mean(ar[1], p[1]), 'ARm': _mean(ar[2], p[2]), 'ARl': _mean(ar[3], p[3])}


def random_set(rng, ncls, nimg, n_det, crowd_rate=0.05, dup_gt=True, ties=True):
    """A seeded evaluation set: images of mixed sizes, ground-truth areas log-uniform over 10 .. 1e5 px^2 (annotation areas that
    differ from the box area), crowd boxes, duplicate boxes, equal confidences, images without ground truth.  Arrays as
    ssd_coco_eval takes them; the detections arrive image by image."""
    sizes = [(640, 480), (480, 640), (500, 375), (1000, 1000), (320, 240)]
    wh = np.array([sizes[int(i)] for i in rng.integers(0, len(sizes), nimg)], np.float64)
    scale = wh[:, 0] * wh[:, 1] / 1e6
    gb, gk, gs, gf, ga = [], [], [], [], []
    for s in range(nimg):
        for _ in range(int(rng.integers(0, 6))):
            area = float(10.0 ** rng.uniform(1, 5))                   # px^2
            side = np.sqrt(area / scale[s])                           # on the grid
            w = max(2, int(side * rng.uniform(0.6, 1.6))); h = max(2, int(side * side / w))
            x0 = int(rng.integers(0, max(1, 1000 - w))); y0 = int(rng.integers(0, max(1, 1000 - h)))
            k = int(rng.integers(0, ncls))
            is_crowd = rng.random() < crowd_rate
            for _rep in range(2 if dup_gt and rng.random() < 0.2 else 1):
                gb.append([x0, x0 + w, y0, y0 + h]); gk.append(k); gs.append(s); gf.append(3 if is_crowd else 0)
                ga.append(float(w * h * scale[s] * rng.uniform(0.5, 1.0)))
    gb = np.array(gb, np.float64).reshape(-1, 4); gs_a = np.array(gs, np.int64)
    db, dk, ds = [], [], []
    per = [n_det // nimg + (1 if s < n_det % nimg else 0) for s in range(nimg)]
    for s in range(nimg):
        rows = np.nonzero(gs_a == s)[0]
        for _ in range(per[s]):
            if len(rows) and rng.random() < 0.6:
                g = int(rows[int(rng.integers(0, len(rows)))])
                j = rng.integers(-1, 2, 4) * rng.integers(0, max(2, int(0.15 * (gb[g, 1] - gb[g, 0]))) + 1, 4)
                db.append(gb[g] + j); dk.append(gk[g] if rng.random() < 0.85 else int(rng.integers(0, ncls)))
            else:
                w, h = (int(v) for v in rng.integers(0, 300, 2)); x0, y0 = (int(v) for v in rng.integers(0, 700, 2))
                db.append([x0, x0 + w, y0, y0 + h]); dk.append(int(rng.integers(0, ncls)))
            ds.append(s)
    n = len(db)
    conf = (rng.integers(1, 200, n) / 200.0) if ties else (rng.permutation(n) + 1) / (n + 1.0)
    return dict(det_box=np.array(db, np.float32).reshape(-1, 4), det_conf=np.asarray(conf, np.float32), det_cls=np.array(dk, np.int32),
                det_sample=np.array(ds, np.int32), gt_box=gb, gt_cls=np.array(gk, np.int32), gt_sample=np.array(gs, np.int32),
                gt_flags=np.array(gf, np.uint8), gt_area=np.array(ga, np.float64), sample_scale=scale, ncls=ncls)


def evaluate_set(s, thresholds=DEFAULT_THRESHOLDS, **kw):
    return evaluate(s['det_box'], s['det_conf'], s['det_cls'], s['det_sample'], s['gt_box'], s['gt_cls'], s['gt_sample'], s['gt_flags'],
                    s['gt_area'], s['sample_scale'], s['ncls'], thresholds, **kw)
