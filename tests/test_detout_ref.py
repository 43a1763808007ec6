"""tests/detout_ref.py without a GPU: for one class and at most nms_top_k candidates the oracle is oracle.boxes.detect, the
cases of the GPU tests have the properties their names promise, and they SEE the bugs the exact comparison is for: every
mutant of the oracle gives another result on at least the case named beside it."""
import numpy as np
import pytest

import detout_cases as dc
import detout_ref as dr
from oracle import boxes as ob


def test_one_class_equals_the_argmax_oracle():
    pname, pred, thr, k, keep = dc.case('one-class')
    anch = dc.anchors(pname)
    assert pred.shape[2] == 6
    for i in range(pred.shape[0]):
        assert int((~(pred[i, :, 0] < np.float32(thr))).sum()) <= k
        want = ob.detect(pred[i], anch, thr, cap=None, max_out=keep)
        assert len(want['idx']) > 50
        assert dr.same(dc.expected('one-class')[i], want)


def test_the_cases_hold_what_their_names_say():
    thr = np.float32(0.01)
    _, pred, _, k, _ = dc.case('counts-k-1-k-k+1')
    assert [int((~(pred[i, :, 0] < thr)).sum()) for i in range(3)] == [k - 1, k, k + 1]
    assert not (~(pred[:, :, 1:3] < thr)).any()
    _, pred, _, k, _ = dc.case('cut-ties')
    col = pred[0, :, 2]
    cand = np.nonzero(~(col < thr))[0]
    assert len(cand) == k + 5 and int((col[cand] == col[cand].min()).sum()) == 10
    tied = cand[col[cand] == col[cand].min()]
    got = dc.expected('cut-ties')[0]
    assert set(tied[5:]).isdisjoint(got['idx']) and set(tied[:5]) & set(got['idx'])        # the 5 lowest anchors of the 10 stay in play
    _, pred, _, k, _ = dc.case('all-equal')
    assert len(np.unique(pred[:, :, 1])) == 1
    for e in dc.expected('all-equal'):
        assert e['idx'][e['cls'] == 1].max() < k
    _, pred, _, _, _ = dc.case('sparse')
    n = (~(pred[..., :3] < thr)).sum((1, 2))
    assert 100 < n[0] < 1000 and n[1] == 0 and 100 < n[2] < 1000
    assert (pred[0, :, :3] == thr).any()
    assert [len(e['idx']) for e in dc.expected('thr-above-all')] == [0, 0]
    _, pred, thr0, _, _ = dc.case('thr-0')
    assert thr0 == 0.0 and (~(pred[..., :2] < 0)).all()
    # more than nms_top_k candidates per class: the select path; an anchor under two classes in one output
    _, pred, _, k, _ = dc.case('softmax-C3')
    assert ((~(pred[..., :3] < thr)).sum(1) > k).all()
    e = dc.expected('sparse')[2]
    assert len(e['idx']) > len(set(e['idx'].tolist()))
    # the final ties sit where keep_top_k = 1 and 2 cut
    e = dc.expected('keep-top-k-1024')[0]
    assert e['conf'][0] == e['conf'][1] and (e['idx'][0], e['cls'][0], e['idx'][1], e['cls'][1]) == (200, 2, 6000, 0)
    assert e['conf'][2] == e['conf'][3] and (e['idx'][2], e['cls'][2], e['idx'][3], e['cls'][3]) == (3000, 0, 3000, 1)
    assert e['conf'][4] == e['conf'][5] and (e['idx'][4], e['cls'][4], e['idx'][5], e['cls'][5]) == (100, 1, 8000, 1)
    assert len(e['idx']) > 200


SEEN_BY = [('threshold_gt', 'sparse'), ('nms_top_k_off_by_one', 'counts-k-1-k-k+1'), ('nms_top_k_off_by_one', 'nms-top-k-1'),
           ('nms_top_k_plus_one', 'counts-k-1-k-k+1'), ('cut_ties_by_higher_anchor', 'cut-ties'), ('cut_ties_by_higher_anchor', 'all-equal'),
           ('keep_top_k_before_nms', 'softmax-C3'), ('class_agnostic_nms', 'softmax-C3'), ('class_agnostic_nms', 'softmax-C28'),
           ('final_ties_by_class_first', 'keep-top-k-1'), ('final_ties_by_class_first', 'keep-top-k-200'),
           ('background_admitted', 'softmax-C1'), ('background_admitted', 'softmax-vgg512-C3')]


def test_every_mutant_is_listed():
    assert {m for m, _ in SEEN_BY} == set(dr.MUTANTS)
    assert {c for _, c in SEEN_BY} <= set(dc.NAMES)


@pytest.mark.parametrize('mutant,name', SEEN_BY, ids=['%s-%s' % mc for mc in SEEN_BY])
def test_the_cases_see_the_mutant(mutant, name):
    good, bad = dc.expected(name), dc.expected(name, mutant)
    assert not all(dr.same(g, m) for g, m in zip(good, bad))
