"""CPU: the COCO box-evaluation oracle (tests/coco_ref.py) on hand-worked cases, the mutations each of which changes at least one
hand-worked number, and its agreement with the VOC07 matching of tests/ap_ref.py on their common ground.  All images here are
1000 x 1000 (sample_scale 1.0) unless a case says otherwise: the grid is the pixel grid."""
import numpy as np
import pytest

import ap_ref
import coco_ref as R

FAR = (800, 900, 800, 900)          # overlaps nothing below
G100 = (0, 100, 0, 100)             # 100 x 100 = 10 000 px^2: 'large'


def run(dets, gts, ncls=1, n_samples=1, thresholds=(0.5,), scale=None, mutate=None):
    """dets: (box, conf[, cls[, sample]]); gts: (box[, cls[, sample[, flags[, area]]]]), area None = the box's own"""
    dets = [tuple(d) + (0, 0)[len(d) - 2:] for d in dets]
    gts = [tuple(g) + (0, 0, 0, None)[len(g) - 1:] for g in gts]
    gts.sort(key=lambda g: g[2])
    scale = np.ones(n_samples) if scale is None else np.asarray(scale, np.float64)
    area = [(g[0][1] - g[0][0]) * (g[0][3] - g[0][2]) * scale[g[2]] if g[4] is None else g[4] for g in gts]
    details = {}
    ap, ar, present = R.evaluate([d[0] for d in dets], [d[1] for d in dets], [d[2] for d in dets], [d[3] for d in dets],
                                 [g[0] for g in gts], [g[1] for g in gts], [g[2] for g in gts], [g[3] for g in gts], area, scale, ncls,
                                 thresholds, mutate=mutate, details=details)
    return ap, ar, present, details


def seq(details, k=0, grp=0, t=0):
    return ''.join(details[(k, grp, t)])


# ------------------------------------------------------------------------------------------ the constants of the rule
def test_recall_thresholds_and_epsilon():
    assert all(j * 0.01 == R.REC_THRS[j] for j in range(101)) and len(R.REC_THRS) == 101
    assert R.EPS == 2.0 ** -52
    assert 2.0 + 2.0 ** -52 == 2.0 and 1.0 / (2.0 + 2.0 ** -52) == 0.5      # halfway between 2 and 2 + 2^-51: ties to even
    assert np.array_equal(R.DEFAULT_THRESHOLDS, np.linspace(0.5, 0.95, 10)) and R.DEFAULT_THRESHOLDS[5] == 0.75


# ------------------------------------------------------------------------------------------ hand-worked cases
def case_fp_then_tp(mutate=None):
    """One box; the stray comes first, then the hit.  pr = [0 / (1 + e), 1 / (2 + e)] = [0, 0.5]; from the back [0.5, 0.5];
    rc = [0, 1]: all 101 q are 0.5, their sum is 50.5 exactly, AP = 50.5 / 101 = 0.5.  The box and both detections are 10 000
    px^2: large.  Under small / medium the class is not present."""
    ap, ar, present, d = run([(FAR, 0.9), (G100, 0.8)], [(G100,)], mutate=mutate)
    return dict(seq=seq(d), ap_all=ap[0, 0, 0], ap_large=ap[3, 0, 0], ap_small=ap[1, 0, 0], ar=ar[0, 0, 0], present=present[:, 0].tolist())


def case_crowd_absorbs_three(mutate=None):
    """A crowd region 200 x 200 and three detections 50 x 50 inside it: IoU = 2500 / 2500 = 1 each (union = the detection), all
    matched to the crowd box, all ignored.  One ordinary box, hit last behind a stray: F I I I T, AP 0.5 as above.  (With the full
    union the IoUs are 2500 / 40000: three more false positives, pr of the hit 1 / (5 + e) = 0.2.)"""
    crowd = ((0, 200, 0, 200), 0, 0, 3)
    dets = [(FAR, 0.9), ((10, 60, 10, 60), 0.8), ((70, 120, 10, 60), 0.7), ((10, 60, 70, 120), 0.6), ((500, 600, 500, 600), 0.5)]
    ap, ar, present, d = run(dets, [crowd, ((500, 600, 500, 600),)], mutate=mutate)
    return dict(seq=seq(d), ap=ap[0, 0, 0], ar=ar[0, 0, 0])


def case_equal_iou_last_wins(mutate=None):
    """The upper and the lower half of the first detection: IoU 5000 / 10000 = 0.5 with both; the LATER one (the lower half) is
    matched.  The second detection is the lower half itself: its box is taken, the upper half has IoU 0: a false positive."""
    ap, ar, present, d = run([(G100, 0.9), ((0, 100, 50, 100), 0.8)], [((0, 100, 0, 50),), ((0, 100, 50, 100),)], mutate=mutate)
    return dict(seq=seq(d), ar=ar[0, 0, 0])


def case_ignored_box_of_higher_iou(mutate=None):
    """A detection 100 x 60: IoU 0.6 with the ordinary box, 1.0 with a flagged copy of itself.  The walk reaches the flagged box
    second, holding a non-ignored match: it stops, the detection is a true positive."""
    ap, ar, present, d = run([((0, 100, 0, 60), 0.9)], [(G100,), ((0, 100, 0, 60), 0, 0, 1)], mutate=mutate)
    return dict(seq=seq(d), ar=ar[0, 0, 0])


def case_area_boundaries(mutate=None):
    """Class 0: a box of annotated area exactly 1024: all, small and medium.  Class 1: exactly 9216: all, medium and large.
    (Both boxes measure 10 000 px^2 on the grid.)"""
    ap, ar, present, d = run([], [(G100, 0, 0, 0, 1024.0), ((200, 300, 200, 300), 1, 0, 0, 9216.0)], ncls=2, mutate=mutate)
    return dict(present0=present[:, 0].tolist(), present1=present[:, 1].tolist())


def case_detection_outside_range(mutate=None):
    """A box annotated with 500 px^2 (small) though it measures 10 000.  Its detection (10 000 px^2, outside small) is matched:
    a true positive under small too.  The stray (10 000 px^2) is unmatched: a false positive under all, ignored under small."""
    ap, ar, present, d = run([(G100, 0.9), (FAR, 0.8)], [(G100, 0, 0, 0, 500.0)], mutate=mutate)
    return dict(all=seq(d, grp=0), small=seq(d, grp=1), present=present[:, 0].tolist())


def case_rank_cap(mutate=None):
    """100 strays in one image, then the hit as the 101st detection of its (image, class): it takes no part.  AR100 = 0."""
    dets = [((300 + i, 400 + i, 300, 400), 0.9 - 0.001 * i) for i in range(100)] + [(G100, 0.1)]
    ap, ar, present, d = run(dets, [(G100,)], mutate=mutate)
    return dict(n=len(d[(0, 0, 0)]), ar100=ar[0, 0, 0], ap=ap[0, 0, 0])


def case_ar_caps(mutate=None):
    """Five boxes in one image; by confidence: hits of boxes 1, 2, 3, seven strays, hits of boxes 4 and 5.  AR1 = 1/5, AR10 = 3/5,
    AR100 = 5/5."""
    boxes = [(150 * i, 150 * i + 100, 0, 100) for i in range(5)]
    dets = [(boxes[i], 0.99 - 0.01 * i) for i in range(3)] + [((300 + i, 400 + i, 500, 600), 0.9 - 0.01 * i) for i in range(7)]
    dets += [(boxes[3], 0.2), (boxes[4], 0.1)]
    ap, ar, present, d = run(dets, [(b,) for b in boxes], mutate=mutate)
    return dict(ar1=ar[4, 0, 0], ar10=ar[5, 0, 0], ar100=ar[0, 0, 0], top1=seq(d, grp=4), top10=seq(d, grp=5))


def case_iou_exactly_at_threshold(mutate=None):
    """The upper half of the box: IoU 5000 / 10000 = 0.5 = the threshold: matched (>=)."""
    ap, ar, present, d = run([((0, 100, 0, 50), 0.9)], [(G100,)], mutate=mutate)
    return dict(seq=seq(d), ar=ar[0, 0, 0])


def case_continuous_iou(mutate=None):
    """A 9 x 9 box and a 9 x 4 detection inside it: 36 / 81 = 0.444: a false positive.  (In the +1 form 10 * 5 / 100 = 0.5: a hit.)"""
    ap, ar, present, d = run([((0, 9, 0, 4), 0.9)], [((0, 9, 0, 9),)], mutate=mutate)
    return dict(seq=seq(d), ar=ar[0, 0, 0])


CASES = {
    case_fp_then_tp: dict(seq='FT', ap_all=0.5, ap_large=0.5, ap_small=-1.0, ar=1.0, present=[1, 0, 0, 1]),
    case_crowd_absorbs_three: dict(seq='FIIIT', ap=0.5, ar=1.0),
    case_equal_iou_last_wins: dict(seq='TF', ar=0.5),
    case_ignored_box_of_higher_iou: dict(seq='T', ar=1.0),
    case_area_boundaries: dict(present0=[1, 1, 1, 0], present1=[1, 0, 1, 1]),
    case_detection_outside_range: dict(all='TF', small='TI', present=[1, 1, 0, 0]),
    case_rank_cap: dict(n=100, ar100=0.0, ap=0.0),
    case_ar_caps: dict(ar1=0.2, ar10=0.6, ar100=1.0, top1='T', top10='TTTFFFFFFF'),
    case_iou_exactly_at_threshold: dict(seq='T', ar=1.0),
    case_continuous_iou: dict(seq='F', ar=0.0),
}


@pytest.mark.parametrize('case', list(CASES), ids=lambda c: c.__name__)
def test_hand_worked(case):
    assert case() == CASES[case]


def test_class_with_only_crowd_boxes_is_not_present():
    ap, ar, present, _ = run([((0, 50, 0, 50), 0.9, 1)], [(G100, 0), ((0, 200, 0, 200), 1, 0, 3)], ncls=2)
    assert present[:, 1].tolist() == [0, 0, 0, 0] and (ap[:, :, 1] == -1.0).all() and (ar[:, :, 1] == -1.0).all()
    assert present[:, 0].tolist() == [1, 0, 0, 1] and ap[0, 0, 0] == 0.0 and ar[0, 0, 0] == 0.0      # class 0: a box, no detection
    s = R.summarize(ap, ar, present, (0.5,))
    assert s['AP'] == 0.0 and s['AP50'] == 0.0 and s['AP75'] == -1.0 and s['APs'] == -1.0 and s['ARl'] == 0.0


def test_empty_evaluation_gives_minus_one():
    ap, ar, present, _ = run([], [], ncls=3, n_samples=0)
    s = R.summarize(ap, ar, present, (0.5,))
    assert list(s) == list(R.SUMMARY_NAMES) and all(v == -1.0 for v in s.values())


def test_summary_numbers_on_two_classes():
    """class 0: the FT case (AP 0.5, AR 1); class 1: a box without detections (AP 0, AR 0): every mean over both is the half"""
    ap, ar, present, _ = run([(FAR, 0.9), (G100, 0.8)], [(G100, 0), ((300, 400, 300, 400), 1)], ncls=2, thresholds=(0.5, 0.75))
    s = R.summarize(ap, ar, present, (0.5, 0.75))
    assert s == dict(AP=0.25, AP50=0.25, AP75=0.25, APs=-1.0, APm=-1.0, APl=0.25, AR1=0.0, AR10=0.5, AR100=0.5, ARs=-1.0, ARm=-1.0, ARl=0.5)


# ------------------------------------------------------------------------------------------ mutations
MUTANT_KILLS = {'strict_threshold': case_iou_exactly_at_threshold, 'first_on_ties': case_equal_iou_last_wins,
                'plus_one_iou': case_continuous_iou, 'crowd_full_union': case_crowd_absorbs_three, 'no_rank_cap': case_rank_cap,
                'box_area_ranges': case_area_boundaries}


def test_every_mutation_is_listed():
    assert set(MUTANT_KILLS) == set(R.MUTATIONS)


@pytest.mark.parametrize('mutation', R.MUTATIONS)
def test_mutation_changes_a_hand_worked_number(mutation):
    case = MUTANT_KILLS[mutation]
    assert case() == CASES[case] and case(mutate=mutation) != CASES[case]


def test_mutants_in_detail():
    assert case_iou_exactly_at_threshold('strict_threshold')['seq'] == 'F'
    assert case_equal_iou_last_wins('first_on_ties') == dict(seq='TT', ar=1.0)
    assert case_continuous_iou('plus_one_iou')['seq'] == 'T'
    mutant = case_crowd_absorbs_three('crowd_full_union')      # every q is 1 / (5 + 2^-52) = 0.2; their sequential sum rounds
    assert mutant['seq'] == 'FFFFT' and mutant['ar'] == 1.0 and abs(mutant['ap'] - 0.2) < 1e-15
    assert case_rank_cap('no_rank_cap')['ar100'] == 1.0
    assert case_area_boundaries('box_area_ranges') == dict(present0=[1, 0, 0, 1], present1=[1, 0, 0, 1])


# ------------------------------------------------------------------------------------------ common ground with VOC07
def test_matching_agrees_with_voc07_on_common_ground(monkeypatch):
    """No flags, area all, one threshold, every IoU far from it, at most one detection per box and strays that touch nothing:
    the continuous and the +1 IoU decide alike and no rule of either protocol but the greedy matching is exercised, so the
    TP / FP sequence of every class must be the one tests/ap_ref.py's VOC07 matching produces.  That module hands its curve
    (one point per detection here: nothing is flagged) to its 11-point form, where this test reads it: a detection is a true
    positive where the recall rises."""
    rng = np.random.default_rng(5)
    ncls, nimg = 3, 12
    dets, gts = [], []
    for s in range(nimg):
        for j in range(int(rng.integers(1, 4))):
            x0, y0 = 250 * j, int(rng.integers(0, 500)); w, h = (int(v) for v in rng.integers(100, 200, 2))
            k = int(rng.integers(0, ncls))
            gts.append(((x0, x0 + w, y0, y0 + h), k, s))
            u = rng.random()
            if u < 0.5:
                dets.append(((x0 + 3, x0 + w - 2, y0 + 1, y0 + h + 4), k, s))                # IoU > 0.8
            elif u < 0.8:
                dets.append(((x0 + w - 20, x0 + 2 * w - 20, y0, y0 + h), k, s))              # IoU < 0.15
        for _ in range(int(rng.integers(0, 3))):
            dets.append(((0, 150, 800, 950), int(rng.integers(0, ncls)), s))                 # below every box
    conf = (rng.permutation(len(dets)) + 1) / (len(dets) + 1.0)
    d = [(b, float(c), k, s) for (b, k, s), c in zip(dets, conf)]
    ap, ar, present, details = run(d, gts, ncls=ncls, n_samples=nimg)
    curves = []
    eleven = ap_ref.eleven_point_fast
    monkeypatch.setattr(ap_ref, 'eleven_point_fast', lambda recall, prec: (curves.append(list(recall)), eleven(recall, prec))[1])
    want, want_present = ap_ref.compute([x[0] for x in d], [x[1] for x in d], [x[2] for x in d], [x[3] for x in d], [g[0] for g in gts],
                                        [g[1] for g in gts], [g[2] for g in gts], ncls=ncls, protocol=ap_ref.VOC07)
    assert np.array_equal(present[0], want_present) and present[0].all() and len(curves) == ncls      # (classes in order, one threshold)
    n_tp = 0
    for k in range(ncls):
        voc07 = ''.join('T' if r > (curves[k][i - 1] if i else 0.0) else 'F' for i, r in enumerate(curves[k]))
        assert ''.join(details[(k, 0, 0)]) == voc07 and len(voc07) == sum(1 for x in d if x[2] == k)
        npos = sum(1 for g in gts if g[1] == k)
        tp = fp = 0.0
        recall, prec = [], []
        for c in details[(k, 0, 0)]:
            assert c in 'TF'
            tp, fp = (tp + 1.0, fp) if c == 'T' else (tp, fp + 1.0)
            recall.append(tp / npos); prec.append(tp / (tp + fp))
        n_tp += int(tp)
        assert ap_ref.eleven_point(recall, prec) == want[0, k]
    assert 5 < n_tp < len(d) - 5


def test_random_set_has_the_awkward_cases():
    s = R.random_set(np.random.default_rng(2), 20, 16, 2000)
    assert len(s['det_conf']) == 2000 and (s['gt_flags'] == 3).any() and len(np.unique(s['det_conf'])) < 200
    assert (np.diff(s['gt_sample']) >= 0).all() and len(set(s['sample_scale'].tolist())) > 2
    ap, ar, present = R.evaluate_set(s)
    assert ap.shape == (4, 10, 20) and ar.shape == (6, 10, 20) and present.shape == (4, 20)
    assert present[1:].sum() > 10 and ap[0][:, present[0] > 0].max() > 0.3 and (ap[1][:, present[1] == 0] == -1.0).all()
    assert (ar[4][:, present[0] > 0] <= ar[5][:, present[0] > 0]).all() and (ar[5][:, present[0] > 0] <= ar[0][:, present[0] > 0]).all()
