"""CPU checks of tests/decode_cases.py, with the oracle alone (no GPU, no library): every case really reaches the edge its
`edge` dict names, expected() is deterministic, and each family tells the mistake it aims at from the right answer -- shown
with `ref()`, a second restatement of decode + NMS in which one decision at a time can be switched (a tie order by higher
anchor, > for >= at the threshold, the last maximum of a row, >= in the suppression test, the `hi` mask of nms_segment
ignored).  Unswitched, ref() must equal expected() on every case."""
import numpy as np
import pytest

import decode_cases as dc
from oracle import boxes as ob

F32 = np.float32
FIELDS = ('idx', 'cls', 'conf', 'box')


def _same(a, b):
    return a['count'] == b['count'] and all(np.array_equal(a[k], b[k]) for k in FIELDS) and \
        np.array_equal(a['conf'].view(np.uint32), b['conf'].view(np.uint32))


def _overlap_sign(rt, i, j):
    """20 inter - 9 union of two round-tripped boxes"""
    w = max(0, min(rt[i, 1], rt[j, 1]) - max(rt[i, 0], rt[j, 0]) + 1)
    h = max(0, min(rt[i, 3], rt[j, 3]) - max(rt[i, 2], rt[j, 2]) + 1)
    inter = w * h
    area = lambda b: (b[1] - b[0] + 1) * (b[3] - b[2] + 1)
    return int(20 * inter - 9 * (area(rt[i]) + area(rt[j]) - inter))


def _nms(box, mutant):
    """greedy NMS over boxes in confidence order -> kept positions.  'sup-ge': >= in the test; 'no-hi': in a segment of 33..64
    boxes the pivots 32.. suppress nothing (nms_segment's second mask dropped)."""
    rt = ob.nms_roundtrip(box)
    n = len(rt)
    area = (rt[:, 1] - rt[:, 0] + 1) * (rt[:, 3] - rt[:, 2] + 1)
    alive = np.ones(n, bool)
    for i in range(n):
        if not alive[i] or (mutant == 'no-hi' and 32 < n <= 64 and i >= 32):
            continue
        j = np.arange(i + 1, n)
        w = np.maximum(0, np.minimum(rt[i, 1], rt[j, 1]) - np.maximum(rt[i, 0], rt[j, 0]) + 1)
        h = np.maximum(0, np.minimum(rt[i, 3], rt[j, 3]) - np.maximum(rt[i, 2], rt[j, 2]) + 1)
        inter = w * h
        union = area[i] + area[j] - inter
        alive[j[(20 * inter >= 9 * union) if mutant == 'sup-ge' else (20 * inter > 9 * union)]] = False
    return np.nonzero(alive)[0]


def ref(case, mutant=None):
    pred, C = case.pred, case.C
    A = pred.shape[0]
    fg = pred[:, :C]
    cls = C - 1 - np.argmax(fg[:, ::-1], axis=1) if mutant == 'last-argmax' else np.argmax(fg, axis=1)
    conf = fg[np.arange(A), cls]
    thr = F32(case.thr)
    cand = np.nonzero(conf > thr if mutant == 'thr-gt' else conf >= thr)[0]
    order = cand[np.lexsort((-cand if mutant == 'tie-high-anchor' else cand, -conf[cand].astype(np.float64)))]
    if case.cap is not None:
        order = order[:case.cap]
    det = dc.decoded(case)
    table = np.zeros((A, 4), np.int64)
    table[det['idx']] = det['box']
    box = table[order]
    if case.nms:
        seen, keep = [], []
        for c in cls[order]:
            if c not in seen:
                seen.append(c)
        for c in seen:
            pos = np.nonzero(cls[order] == c)[0]
            keep.extend(pos[_nms(box[pos], mutant)])
        keep = np.array(keep, np.int64)
    else:
        keep = np.arange(len(order))
    keep = keep[:case.max_out]
    order = order[keep]
    return dict(count=len(order), idx=order, cls=cls[order], conf=conf[order], box=box[keep])


ALL = dc.all_cases()
IDS = ['%s-C%d-%s' % (c.pname, c.C, c.name) for c in ALL]


def _by_family(family, pname=None, C=None):
    return [c for c in ALL if c.edge.get('family') == family and (pname is None or c.pname == pname) and (C is None or c.C == C)]


def test_every_combination_has_its_cases_and_batches_hold_each_once():
    for pname, C in dc.COMBOS:
        cs = dc.cases(pname, C)
        groups = dc.batches(pname, C)
        placed = [c for _, g in groups for c in g]
        assert sorted(c.name for c in set(placed)) == sorted(c.name for c in cs)
        for params, g in groups:
            assert all(c.params == params for c in g)
        main = max(groups, key=lambda pg: len(pg[1]))[1]
        names = [c.name for c in main]
        k = names.index('count-0-nms')
        assert names[k - 1] == names[k + 1] == 'count-A-nms'       # an empty image between two full ones
    fams = {c.edge['family'] for c in dc.cases('vgg300', 20)}
    assert fams == {'counts', 'caps', 'max_out', 'out_cap', 'ties', 'ties-cap', 'ties-class-order', 'threshold', 'argmax', 'segments',
                    'iou-line', 'box-arith'}


@pytest.mark.parametrize('case', ALL, ids=IDS)
def test_ref_equals_expected_and_expected_is_deterministic(case):
    want = dc.expected(case)
    assert _same(want, dc.expected(case))
    assert _same(ref(case), want)
    assert want['idx'].dtype == np.int64 and want['conf'].dtype == F32 and want['box'].shape == (want['count'], 4)


def test_decoded_is_recomputed_identically():
    case = next(c for c in ALL if c.name == 'segment-65-broken')
    first = dc.expected(case)
    dc._DECODED.clear()
    assert _same(first, dc.expected(case))


@pytest.mark.parametrize('case', [c for c in ALL if c.edge['family'] in ('counts', 'caps')], ids=lambda c: '%s-C%d-%s' % (c.pname, c.C, c.name))
def test_counts_and_caps(case):
    det = dc.decoded(case)
    n = case.edge['n']
    assert len(det['idx']) == n
    assert len(np.unique(det['conf'])) == n                       # distinct confidences
    if n >= case.C:
        assert len(np.unique(det['cls'])) == case.C               # spread over all classes
    want = dc.expected(case)
    if case.edge['family'] == 'caps':
        assert case.edge['m'] == min(n, case.cap)
        assert want['count'] <= case.edge['m'] and (case.nms or want['count'] == case.edge['m'])
        if case.edge['m'] and case.nms:
            assert 0 < want['count'] < case.edge['m'] or case.edge['m'] == 1      # the suppression does something
    elif not case.nms:
        assert want['count'] == n
    elif n > 64:
        assert 0 < want['count'] < n


def test_max_out_and_out_cap():
    cs = _by_family('max_out') + _by_family('out_cap')
    assert len(cs) == 8
    s = cs[0].edge['survivors']
    assert sorted(c.max_out for c in cs if c.edge['family'] == 'max_out' and c.nms) == [0, 1, s - 1, s, s + 1] and s > 8
    for c in cs:
        want = dc.expected(c)
        assert want['count'] == c.edge['count']
        if c.edge['family'] == 'out_cap':
            assert c.out_cap < want['count']


@pytest.mark.parametrize('case', _by_family('ties') + _by_family('ties-cap'), ids=lambda c: '%s-C%d-%s' % (c.pname, c.C, c.name))
def test_ties(case):
    det = dc.decoded(case)
    assert len(det['idx']) == case.edge['n']
    assert set(np.unique(det['conf'])) <= {F32(k / 8) for k in range(1, 9)}
    runs = np.unique(det['conf'], return_counts=True)[1]
    assert int((runs * (runs - 1) // 2).sum()) > 1000                      # tied pairs
    same = det['conf'][1:] == det['conf'][:-1]
    assert np.all(det['idx'][1:][same] > det['idx'][:-1][same])           # lower anchor first
    if case.edge['n'] == dc.A_OF[case.pname] and case.C == 20:
        longest = int(np.bincount(det['cls']).max())
        assert longest > (400 if case.pname == 'vgg300' else 1100)          # class segments far beyond one wave
    if case.edge['family'] == 'ties-cap':
        a, b = dc.cut_in_run(case)
        assert a == b
    assert not _same(ref(case, 'tie-high-anchor'), dc.expected(case))


def test_ties_class_order():
    cs = _by_family('ties-class-order')
    assert cs
    for c in cs:
        cls = list(dc.expected(c)['cls'])
        assert [k for i, k in enumerate(cls) if k not in cls[:i]] == c.edge['group_order']
        assert not _same(ref(c, 'tie-high-anchor'), dc.expected(c))


@pytest.mark.parametrize('case', _by_family('threshold'), ids=lambda c: '%s-C%d-%s' % (c.pname, c.C, c.name))
def test_threshold(case):
    det = dc.decoded(case)
    e = case.edge
    assert len(det['idx']) == e['n']
    assert len(e['at']) >= 30 and len(e['just_above']) == 30
    assert np.all(case.pred[e['at']].max(1, initial=0, where=np.arange(case.C + 5) < case.C) == F32(case.thr))
    assert np.isin(e['at'], det['idx']).all() and np.isin(e['just_above'], det['idx']).all()
    assert not np.isin(e['just_below'], det['idx']).any()
    if case.thr > 0:
        assert len(e['just_below']) == 30
    else:
        above = det['conf'][np.isin(det['idx'], e['just_above'])]
        assert np.all(above.view(np.uint32) == 1) and np.all(det['cls'][np.isin(det['idx'], e['just_above'])] == 1)
    assert not _same(ref(case, 'thr-gt'), dc.expected(case))


@pytest.mark.parametrize('case', _by_family('argmax'), ids=lambda c: '%s-C%d-%s' % (c.pname, c.C, c.name))
def test_argmax(case):
    det = dc.decoded(case)
    e = case.edge
    where = {int(a): k for k, a in enumerate(det['idx'])}
    for row, c in e['want'].items():
        assert det['cls'][where[row]] == c, row
    for row, c in e['background'].items():
        assert case.pred[row, case.C] >= case.pred[row, :case.C].max() and row in where
    assert e['not_candidate'] not in where
    if case.C >= 2:
        assert not _same(ref(case, 'last-argmax'), dc.expected(case))
    if case.C >= 28:
        combos = {(a % 4, b % 4) for a, b in e['pairs']} | {(b % 4, a % 4) for a, b in e['pairs']}
        assert len({(a % 4, b % 4) for a, b in e['pairs']}) == 16 and len(combos) == 16
        assert any(b == case.C - 1 for a, b in e['pairs'])
    if case.C == 127:
        assert any(a >= 28 for a, b in e['pairs'])


@pytest.mark.parametrize('case', _by_family('segments'), ids=lambda c: '%s-C%d-%s' % (c.pname, c.C, c.name))
def test_segments(case):
    e = case.edge
    det = dc.decoded(case)
    L, cc = e['L'], e['chain_cls']
    counts = np.bincount(det['cls'], minlength=case.C)
    assert counts[cc] == L and all(counts[c] == ln for c, ln in e['others'].items()) and counts.sum() == e['n']
    if e['others']:
        assert det['cls'][0] != cc                                   # the chain is not the first segment
    chain = det['idx'][det['cls'] == cc]
    assert np.array_equal(chain, e['chain_rows'])                    # confidence order == chain order
    want = dc.expected(case)
    kept = want['idx'][want['cls'] == cc]
    if L <= 100:
        rt = ob.nms_roundtrip(det['box'][det['cls'] == cc])
        for k in range(L - 1):
            assert (_overlap_sign(rt, k, k + 1) > 0) == (k not in e['breaks']), k
            if k + 2 < L:
                assert _overlap_sign(rt, k, k + 2) < 0, k
        surv = dc.chain_survivors(L, e['breaks'])
        assert np.array_equal(kept, e['chain_rows'][surv])
        if e['breaks']:
            assert {31, 32, 63, 64} <= set(surv)                     # both sides of the links across lanes 31/32 and 63/64
        else:
            assert surv == list(range(0, L, 2))
    else:
        assert 0 < len(kept) < L
    differs = not _same(ref(case, 'no-hi'), want)
    assert differs == (34 <= L <= 64), L                             # pivot 32, the first of `hi`, needs a box behind it


def test_iou_on_the_line():
    (case,) = _by_family('iou-line')
    want = dc.expected(case)
    signs = []
    for (a, b, d), found in zip(case.edge['pairs'], dc._IOU_LINE_FOUND):
        rt, inter, union, got = dc.pair_boxes(case.pname, a, case.pred[a, case.C + 1:], b, case.pred[b, case.C + 1:])
        assert got == d == found[4] and inter > 0 and abs(d) <= 1000 and abs(d) < 1e-4 * 20 * inter
        assert a in want['idx'] and (b in want['idx']) == (d <= 0)
        signs.append(int(np.sign(d)))
    assert sorted(signs) == [-1, 0, 1]
    assert not _same(ref(case, 'sup-ge'), want)


def test_box_arithmetic():
    (case, dec) = _by_family('box-arith')
    e = case.edge
    C, an = case.C, dc.anchors(case.pname)
    bad = [r for r, (kind, _) in e['kinds'].items() if kind in ('nan', 'centre-neg-inf')]
    assert sorted(bad) == list(e['nonfinite']) and len(bad) >= 11
    with pytest.raises((ValueError, OverflowError)):
        ob.decode(case.pred, an, case.thr, None)                     # the reference's behaviour on such offsets
    det = dc.decoded(case)
    where = {int(a): k for k, a in enumerate(det['idx'])}
    for r in bad:
        assert not det['box'][where[r]].any()
    want = dc.expected(case)
    corner = [i for i in want['idx'] if i in bad]
    assert len(corner) == 2                                           # one per class: the others meet it at IoU 1 and go
    assert sum(1 for i in dc.expected(dec)['idx'] if i in bad) == len(bad)
    seen = set()
    for r, (kind, slot) in e['kinds'].items():
        loc = case.pred[r, C + 1:]
        if kind == 'clamp':
            at100 = loc.copy(); at100[slot] = 100
            box100 = ob.normalize_abs_np2(*ob.decode_location_np2(at100, an[r]))
            assert np.isfinite(np.exp(20.0) * an[r, 2:]).all()
            if loc[slot] >= 100:
                assert tuple(det['box'][where[r]]) == box100
                seen.add(('clamped', slot, float(loc[slot])))
            elif slot < 2 and loc[slot] < 99.9:
                assert tuple(det['box'][where[r]]) != box100         # 99 < offset < 100 is NOT clamped, and it shows
                seen.add(('below', slot))
        elif kind == 'size-zero':
            b = det['box'][where[r]]
            assert b[1] - b[0] <= 1 if slot == 2 else b[3] - b[2] <= 1
        elif kind == 'outside' and abs(loc[slot]) == 1e4:
            b = det['box'][where[r]]
            lo, hi = (b[0], b[1]) if slot == 0 else (b[2], b[3])
            # max is clipped to 999 and min to 0, then min onto max: 999 on the far side, max's own negative value on the near one
            assert lo == hi and (lo == 999 if loc[slot] > 0 else lo < -1000)
            seen.add(('outside', slot, int(np.sign(lo))))
    assert {('below', 0), ('below', 1)} <= seen
    assert {('outside', s, v) for s in (0, 1) for v in (-1, 1)} <= seen
    assert len([s for s in seen if s[0] == 'clamped']) == 16


# ---- ssd_nms_boxes ------------------------------------------------------------------------------------------------------
def _sign_bit_order(boxes, conf, group, thr):
    """the oracle on the order the kernel had before its fix: -0.0 strictly below +0.0 (sign-magnitude bits)"""
    bits = conf.view(np.uint32).astype(np.int64)
    key = np.where(bits >> 31, ~bits & 0xFFFFFFFF, bits | 0x80000000)
    g = np.zeros(len(conf), np.int64) if group is None else group
    order = np.lexsort((np.arange(len(conf)), -key, g))
    pick = []
    for gg in np.unique(g):
        pos = [int(i) for i in order if g[i] == gg]
        sub = ob.nms_list([(1.0 - k, tuple(int(v) for v in boxes[i])) for k, i in enumerate(pos)], thr)      # already in order
        pick.extend(pos[k] for k in sub)
    return pick


def test_nms_box_cases():
    names = []
    for name, boxes, conf, group, thr, edge in dc.nms_cases():
        names.append(name)
        want = dc.nms_expected(boxes, conf, group, thr)
        assert want == dc.nms_expected(boxes, conf, group, thr)
        if 'order' in edge:
            assert want == edge['order'], name
        if name.startswith('zeros'):
            assert np.signbit(conf).any() and (conf == 0).sum() >= 2
            # the old order shows on this case (not on the one where +0.0 comes first anyway)
            assert (_sign_bit_order(boxes, conf, group, thr) != want) == (name != 'zeros-pos-first'), name
        elif len(conf) < 1000:
            assert _sign_bit_order(boxes, conf, group, thr) == want, name
        if name.startswith('ratio'):
            r = ob.nms_roundtrip  # (not applied: these are the integers ssd_nms_boxes takes)
            w = min(boxes[0, 1], boxes[1, 1]) - max(boxes[0, 0], boxes[1, 0]) + 1
            inter = int(w)
            union = int(boxes[0, 1] - boxes[0, 0] + 1 + boxes[1, 1] - boxes[1, 0] + 1 - inter)
            assert (inter, union) == (edge['inter'], edge['union'])
            assert (inter / union > thr) == name.endswith('more')
            if not name.endswith('more'):
                assert inter / union == thr                            # equality in the f64 quotient
        if name == 'own-groups-4096':
            assert len(np.unique(group)) == len(group) == 4096 and len(want) == 4096
        if name == 'clusters-65535':
            assert len(conf) == 65535 and 3 <= len(want) < 200
        if name == 'heavy-ties':
            assert len(np.unique(conf)) <= 5 and (conf < 0).any() and not np.signbit(conf[conf == 0]).any()
    assert len(set(names)) == len(names) and len(names) >= 20
