"""CPU: the numpy oracle of Soft-NMS (tests/softnms_ref.py) against itself -- its identities, expw against float64 exp, the
float64 restatement -- and the cases of the GPU tests (tests/softnms_cases.py): every case reaches the edge it is named for, and
every mutant of the oracle differs from it on at least one of them."""
import numpy as np
import pytest

import detout_cases as dc
import detout_ref as dr
import softnms_cases as sc
import softnms_ref as sr
import tiledet_ref as tdr

F32 = np.float32
KINDS = (sr.LINEAR, sr.GAUSSIAN)


def bits(a):
    return np.asarray(a, F32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ expw
def test_expw_against_float64_exp():
    """Measured on this seeded grid of 2.5 million points of [-87, 0] plus the edges: at most 0.975 ulp from float64 exp (the
    bound held below is 1.5 ulp: the margin is for points the sample misses); never above 1; the smallest value a normal number."""
    rng = np.random.default_rng(38)
    x = np.concatenate([np.linspace(-87.0, 0.0, 1500001), -rng.uniform(0.0, 87.0, 600000), -rng.exponential(1.0, 400000),
                        [0.0, -0.0, -87.0, -1e-30, -1e-45]]).astype(F32)
    x = x[x >= F32(-87.0)]
    y = sr.expw(x)
    exact = np.exp(x.astype(np.float64))
    ulp = np.abs(y.astype(np.float64) - exact) / np.spacing(exact.astype(F32)).astype(np.float64)
    assert ulp.max() <= 1.5, ulp.max()
    assert ulp.max() > 0.5                                   # (a float32 result cannot be exact everywhere: the figure is a real one)
    assert y.max() == F32(1.0) and y.min() >= np.finfo(F32).tiny
    assert bits(sr.expw(np.array([0.0, -0.0], F32))).tolist() == [0x3F800000] * 2
    assert bits(sr.expw(np.array([-87.5, -100.0, -np.inf, np.nextafter(F32(-87), F32(-88))], F32))).tolist() == [0] * 4
    assert np.all(np.diff(sr.expw(np.linspace(-87, 0, 100001).astype(F32)).astype(np.float64)) >= 0)


# ------------------------------------------------------------------------------------------------ identities
@pytest.mark.parametrize('kind', KINDS)
def test_disjoint_boxes_are_a_no_op(kind):
    d = sc.list_case('disjoint')
    order, scores = sc.list_expected('disjoint', kind)
    by_conf = np.lexsort((np.arange(100), -d['conf'].astype(np.float64)))
    assert np.array_equal(order, by_conf) and np.array_equal(bits(scores), bits(d['conf'][by_conf]))


def test_linear_with_iou_thr_1_emits_every_candidate_in_order():
    for name in ('iou-thr-1', 'identical-iou-thr-1'):
        d = sc.list_case(name)
        order, scores = sc.list_expected(name, sr.LINEAR)
        by_conf = np.lexsort((np.arange(len(d['conf'])), -d['conf'].astype(np.float64)))
        assert np.array_equal(order, by_conf) and np.array_equal(bits(scores), bits(d['conf'][by_conf]))


@pytest.mark.parametrize('name', sc.LIST_NAMES)
@pytest.mark.parametrize('kind', KINDS)
def test_emitted_keys_are_strictly_descending(name, kind):
    order, scores = sc.list_expected(name, kind)
    key = (bits(scores).astype(np.uint64) << np.uint64(32)) | ((32767 - order).astype(np.uint64) << np.uint64(8))
    assert np.all(key[1:] < key[:-1])
    assert len(set(order.tolist())) == len(order)
    mn = F32(sc.list_case(name)['params'][kind][2])
    assert np.all(scores >= mn)


@pytest.mark.parametrize('name', [n for n in dc.NAMES if n != 'softmax-C127'])
def test_kind_hard_equals_detout_ref(name):
    """the hard rule run through the soft oracle's loop (pick the largest remaining key, a weight of 0 removes) and its own
    restatement of steps 1, 2 and 4 is tests/detout_ref.py's result on every one of its cases"""
    pname, pred, thr, k, keep = dc.case(name)
    got = [sr.detection_output(pred[i], dc.anchors(pname), thr, k, keep, sr.HARD) for i in range(pred.shape[0])]
    assert all(dr.same(g, w) for g, w in zip(got, dc.expected(name)))


def test_kind_hard_equals_tiledet_ref():
    pname, thr, k, keep, m = sc.TILED
    pred, tiles = sc.tiled_case()
    want = tdr.detout_tiles_all(pred, tiles, dc.anchors(pname), thr, k, keep, m)
    assert all(tdr.same(g, w) for g, w in zip(sc.tiled_expected(sr.HARD), want)) and all(len(w['idx']) > 20 for w in want)


def test_image_steps_equal_detout_ref_when_nothing_overlaps():
    """kind aside, steps 1, 2 and 4 are detout_ref's: with iou_thr = 1 (linear) nothing decays and, the hard rule being switched
    off the same way (nms_top_k candidates that never overlap: one candidate per class), the two oracles agree"""
    pname, pred, thr, k, keep = dc.case('nms-top-k-1')
    for i in range(pred.shape[0]):
        assert dr.same(dr.detection_output(pred[i], dc.anchors(pname), thr, 1, keep),
                       sr.detection_output(pred[i], dc.anchors(pname), thr, 1, keep, sr.LINEAR, 1.0))
    pname, pred, thr, k, keep = dc.case('thr-above-all')
    assert len(sr.detection_output(pred[0], dc.anchors(pname), thr, k, keep)['idx']) == 0


@pytest.mark.parametrize('kind', KINDS)
def test_float64_restatement_agrees_to_rounding(kind):
    """the float32 sequence approximates the rule in exact arithmetic: same picks in the same order, scores within a few ulp per
    decay, on a list whose scores are far enough apart that rounding cannot reorder them"""
    d = sc.list_case('overlap-65')
    order, scores = sc.list_expected('overlap-65', kind)
    o64, s64 = sr.soft_nms_f64(d['conf'], (32767 - np.arange(65)) << 8, d['box'], kind, *d['params'][kind])
    assert np.array_equal(order, o64)
    assert np.max(np.abs(scores.astype(np.float64) - s64) / s64) < 65 * 4 * 2.0 ** -24


# ------------------------------------------------------------------------------------------------ the cases reach their edges
def test_list_cases_reach_the_edges_they_are_named_for():
    for n in sc.SIZES:
        assert len(sc.list_case(f'overlap-{n}')['conf']) == n
        for kind in KINDS:
            order, scores = sc.list_expected(f'overlap-{n}', kind)
            conf = sc.list_case(f'overlap-{n}')['conf']
            assert 1 <= len(order) <= n
            if n >= 63:      # picks leave confidence order, scores decay, candidates are dropped
                assert len(order) < n and np.any(bits(scores) != bits(conf[order])) and np.any(np.diff(conf[order].astype(np.float64)) > 0)
            assert order[0] == n - 1                         # the last candidate: the last lane and register slot in use
            if n >= 400:     # picks come from every register slot of a lane
                assert len(set((order // 64).tolist())) > (n + 63) // 128
    for kind in KINDS:
        order, scores = sc.list_expected('identical-equal', kind)
        assert order.tolist() == list(range(70))             # ties by index all the way
        assert scores[0] == F32(0.5) and scores[-1] == 0
    assert np.all(sc.list_expected('identical-equal', sr.LINEAR)[1][1:] == 0)                   # the linear weight is exactly 0
    g = sc.list_expected('identical-equal', sr.GAUSSIAN)[1]
    assert g[1] == F32(0.5) * sr.expw(np.array([-2.0], F32))[0] and 0 < g[2] < g[1]
    for kind in KINDS:
        order, _ = sc.list_expected('equal-conf', kind)
        assert order[0] == 0 and 1 < len(order) < 129
        on, below = sc.list_expected('on-min-score', kind), sc.list_expected('ulp-below-min-score', kind)
        mn = F32(sc.list_case('on-min-score')['params'][kind][2])
        assert on[0].tolist() == [0, 1] and on[1][1] == mn and below[0].tolist() == [0]
        assert np.nextafter(mn, F32(1)) == F32(sc.list_case('ulp-below-min-score')['params'][kind][2])
        assert sc.list_expected('drop-after-first', kind)[0].tolist() == [0]
        assert len(sc.list_expected('iou-thr-0', kind)[0]) > 1
    lin0, lin45 = sc.list_expected('iou-thr-0', sr.LINEAR), sc.list_expected('overlap-129', sr.LINEAR)
    assert len(lin0[0]) < len(lin45[0]) < 129 == len(sc.list_expected('iou-thr-1', sr.LINEAR)[0])
    # sigma 0.01: a weight of exactly 0 (x < -87) and weights that are neither 0 nor 1
    d = sc.list_case('sigma-0.01')
    b = sr.ob.nms_roundtrip(d['box'].astype(np.int64))
    inter, uni = sr.overlap_ints(b[0], b)
    w = sr.weights(inter, uni, sr.GAUSSIAN, 0.45, 0.01)
    assert np.sum(w == 0) >= 10 and np.any((w > 0) & (w < 1))
    assert np.sum(sc.list_expected('sigma-0.01', sr.GAUSSIAN)[1] == 0) >= 9
    for kind in KINDS:
        _, s = sc.list_expected('denormal', kind)
        tiny = np.finfo(F32).tiny
        assert len(s) == 64 and np.sum((s > 0) & (s < tiny)) >= 5, s      # denormal products are kept and emitted


def test_image_cases_reach_the_edges_they_are_named_for():
    for kind in KINDS:
        ff = sc.image_expected('full-frame', kind)
        for w in ff:
            full = np.all(w['box'] == np.array([0, 999, 0, 999]), axis=1)
            # (identical boxes: the linear weight is 0, one of them stays per class; the gaussian keeps more)
            assert full.sum() >= (2 if kind == sr.LINEAR else 4) and len(set(w['cls'][full].tolist())) == 2
        pname, pred, thr, k, keep, _ = sc.image_case('keep-top-k-50')
        all_picks = sr.detection_output(pred[0], dc.anchors(pname), thr, k, 1024, kind)
        assert min(np.bincount(all_picks['cls'], minlength=3)) > 50 and len(sc.image_expected('keep-top-k-50', kind)[0]['idx']) == 50
        above, below = sc.image_expected('min-score-above-thr', kind)[0], sc.image_expected('min-score-below-thr', kind)[0]
        assert 0 < len(above['idx']) < len(below['idx']) < 900 and above['conf'].min() >= F32(0.4)
        assert F32(0.05) <= below['conf'].min() < F32(0.2)      # (both cases: thr = 0.2)
        for name in ('sparse', 'all-equal', 'counts-k-1-k-k+1', 'cut-ties', 'keep-top-k-1024'):      # (every pick is output)
            if True:
                assert any(not dr.same(h, s) for h, s in zip(dc.expected(name), sc.image_expected(name, kind))), name
    assert {dc.case(n)[1].shape[2] - 5 for n in dc.NAMES} >= {1, 27, 28, 127} and dc.case('softmax-vgg512-C3')[0] == 'vgg512'


# ------------------------------------------------------------------------------------------------ the mutants
def _list_differs(name, kind, mutant):
    a, b = sc.list_expected(name, kind), sc.list_expected(name, kind, mutant)
    return not (np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])))


@pytest.mark.parametrize('mutant', sr.MUTANTS)
def test_every_mutant_differs_on_a_case_the_gpu_tests_use(mutant):
    seen = []
    if mutant == 'class_agnostic':
        for kind in KINDS:
            for name in ('full-frame', 'sparse'):
                if any(not dr.same(a, b) for a, b in zip(sc.image_expected(name, kind), sc.image_expected(name, kind, mutant))):
                    seen.append((name, kind))
    else:
        for kind in KINDS:
            seen += [(name, kind) for name in sc.LIST_NAMES if _list_differs(name, kind, mutant)]
    assert seen, mutant
    wanted = {'gaussian_threshold': sr.GAUSSIAN, 'fma_poly': sr.GAUSSIAN, 'linear_ge': sr.LINEAR}
    if mutant in wanted:
        assert all(k == wanted[mutant] for _, k in seen)
    elif mutant != 'iou_f64':
        assert {k for _, k in seen} == set(KINDS), (mutant, seen)      # told apart under both kinds


def test_the_tiled_oracle_sees_tiles_in_the_ties_and_mutants():
    for kind in KINDS:
        want = sc.tiled_expected(kind)
        assert all(100 < len(w['idx']) <= sc.TILED[3] for w in want)
        top = want[0]
        assert top['conf'][0] == top['conf'][1] == F32(0.95) and top['tile'][:2].tolist() == [0, 1]      # equal scores: the lower tile
        for mutant in ('no_rerank', 'ties_by_higher_anchor'):
            other = sc.tiled_expected(kind, mutant)
            assert any(not tdr.same(a, b) for a, b in zip(want, other)), (kind, mutant)
