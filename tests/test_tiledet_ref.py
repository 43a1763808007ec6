"""CPU: the numpy oracle of tiled DetectionOutput (tests/tiledet_ref.py) against the oracles it extends, and the
cases of tests/test_gpu_tiledet.py against its mutants: every plausible wrong rule gives another result on at least one case
the GPU test runs, so the exact comparison there checks the rule."""
import numpy as np
import pytest

import detout_cases as DC
import detout_ref as dr
import tiledet_cases as TC
import tiledet_ref as R
import tiles_ref as tr

# mutant -> the cases that were built to tell it from the oracle
KILLED_BY = {
    'edge_drop_before_cut': ['rules'],
    'nms_inside_tile': ['rules', 'classes-127'],
    'no_picture_cut': ['rules', 'one-class', 'classes-127'],
    'nms_on_tile_grid': ['scene', 'two-pictures', 'vgg512'],
    'cut_ties_by_anchor_before_tile': ['rules'],
    'final_ties_by_class_before_anchor': ['rules'],
    'keep_top_k_per_tile': ['scene-k8-keep5'],
    'class_agnostic_nms': ['scene', 'classes-127'],
}


def _differs(name, mutant):
    return any(not R.same(a, b) for a, b in zip(TC.expected(name), TC.expected(name, mutant)))


def test_every_mutant_has_cases():
    assert set(KILLED_BY) == set(R.MUTANTS)
    assert all(n in TC.NAMES for names in KILLED_BY.values() for n in names)


@pytest.mark.parametrize('mutant', R.MUTANTS)
def test_cases_tell_the_mutant_from_the_oracle(mutant):
    for name in KILLED_BY[mutant]:
        assert _differs(name, mutant), (mutant, name)


def test_rules_case_is_what_its_docstring_says():
    """the planted boxes decode where they were planted: the kept records are the ones the rules name"""
    (got,) = TC.expected('rules')
    rec = sorted(zip(got['cls'].tolist(), got['tile'].tolist(), [float(c) for c in got['conf']]))
    c0 = [(t, c) for k, t, c in rec if k == 3]
    c1 = [(t, c) for k, t, c in rec if k == 1]
    assert sorted(c0) == [(0, np.float32(0.65)), (0, np.float32(0.7)), (0, np.float32(0.8))]
    assert sorted(c1) == [(0, np.float32(0.75)), (0, np.float32(0.9)), (1, np.float32(0.75)), (2, np.float32(0.8))]
    # the two 0.75 of tile 1 have lower anchors than tile 0's, and the kept one is the lower of the two
    pname, pred, tiles, thr, k, keep, m = TC.case('rules')
    a0 = np.nonzero(pred[0, :, 1] == np.float32(0.75))[0]
    a1 = np.nonzero(pred[1, :, 1] == np.float32(0.75))[0]
    assert len(a0) == 1 and len(a1) == 2 and a1.max() < a0[0]
    assert got['idx'][(got['cls'] == 1) & (got['tile'] == 1)].tolist() == [int(a1.min())]
    # the 0.6 pair: (low anchor, class 2) before (high anchor, class 0)
    pair = np.nonzero(got['conf'] == np.float32(0.6))[0]
    assert got['cls'][pair].tolist() == [2, 0] and got['idx'][pair[0]] < got['idx'][pair[1]] and got['tile'][pair].tolist() == [1, 1]


def test_both_picture_cuts_bite_with_ties_at_the_cut():
    pname, pred, tiles, thr, k, keep, m = TC.case('scene-k8-keep5')
    (full,) = R.detout_tiles_all(pred, tiles, TC.anchors(pname), thr, 400, 200, m)
    (got,) = TC.expected('scene-k8-keep5')
    assert len(got['idx']) == keep < len(full['idx'])
    # keep_top_k: the confidence of the last kept record is shared by the first one left out
    (more,) = R.detout_tiles_all(pred, tiles, TC.anchors(pname), thr, k, keep + 1, m)
    assert more['conf'][keep] == got['conf'][keep - 1]
    # nms_top_k: some class has more than k candidates in the picture, the k-th and the (k+1)-th with one confidence
    C = pred.shape[2] - 5
    (uncut,) = R.detout_tiles_all(pred, tiles, TC.anchors(pname), thr, k, 1024, m, mutant='no_picture_cut')
    assert len(uncut['idx']) > len(R.detout_tiles_all(pred, tiles, TC.anchors(pname), thr, k, 1024, m)[0]['idx'])
    tied = 0
    for c in range(C):
        confs = np.sort(np.concatenate([np.sort(pred[t, :, c][~(pred[t, :, c] < np.float32(thr))])[::-1][:k] for t in range(len(tiles))]))[::-1]
        tied += len(confs) > k and confs[k - 1] == confs[k]
    assert tied > 0


def test_keys_order_as_the_rules():
    (got,) = TC.expected('scene')
    keys = [R.key(c, t, a, k) for c, t, a, k in zip(got['conf'], got['tile'], got['idx'], got['cls'])]
    assert len(keys) > 20 and keys == sorted(keys, reverse=True) and len(set(keys)) == len(keys)
    assert len(set(got['conf'].tolist())) < len(keys)                                  # ties occur


@pytest.mark.parametrize('name', ['sparse', 'softmax-C3', 'cut-ties', 'keep-top-k-2'])
def test_one_tile_picture_equals_detection_output(name):
    pname, pred, thr, k, keep = DC.case(name)
    want = DC.expected(name)
    for i in range(pred.shape[0]):
        got = R.detout_tiles(pred[i:i + 1], [(0, 0, 640, 480, 0)], (640, 480), DC.anchors(pname), thr, k, keep, 2)
        assert dr.same(got, want[i]) and not got['tile'].any(), (name, i)


def test_plan_tiles_interior_bits():
    tiles = tr.plan_tiles_ref(1000, 700, 400)
    assert tiles == [(0, 0, 400, 400, 2 | 8), (300, 0, 400, 400, 1 | 2 | 8), (600, 0, 400, 400, 1 | 8),
                     (0, 300, 400, 400, 2 | 4), (300, 300, 400, 400, 1 | 2 | 4), (600, 300, 400, 400, 1 | 4), (0, 0, 1000, 700, 0)]
    assert [t[1] for t in TC.case('scene')[2]] == tiles
    assert tr.plan_tiles_ref(300, 200, 400) == [(0, 0, 300, 200, 0)]
    from ssd_tensorflow_amd import tiling
    assert [tuple(t) for t in tiling.plan_tiles(1000, 700, 400)] == tiles
    assert [tuple(t) for t in tiling.plan_tiles(700, 400, 400)] == [t[1] for t in TC.case('one-class')[2]]


def test_empty_and_dropped_pictures():
    got = TC.expected('empty-and-dropped')
    assert [len(g['idx']) for g in got] == [0, 0, 1]
    assert len(R.detout_tiles_all(*TC.case('empty-and-dropped')[1:3], TC.anchors('vgg300'), 0.01, 400, 200, -1)[1]['idx']) > 0


def test_many_tiles_case():
    (got,) = TC.expected('tiles-256')
    # three 0.75 lead (tiles 17, 100, 255 in that order); the cut at 3 leaves nothing else
    assert got['tile'].tolist() == [17, 100, 255] and (got['conf'] == np.float32(0.75)).all()
