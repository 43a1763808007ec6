"""-m gpu: the label encoder's matching rules through the host, _dev and resident forms of the C ABI,
against the numpy oracle of tests/match_ref.py: the matching itself (match_out) and the class columns byte for byte,
the offsets within the label tolerance of tests/test_gpu_boxes.py (the device's f64 log may differ from libm in the
last ulp before the f32 cast)."""
import functools

import numpy as np
import pytest

import match_ref as mr
from oracle import boxes as ob
from match_cases import HAND_CASES
from ssd_tensorflow_amd import _lib, ssdutils as su
from ssd_tensorflow_amd._lib import lib, check, np_ptr

pytestmark = pytest.mark.gpu
FORMS = ['host', 'dev', 'resident']
RULES = {'reference': 0, 'paper': 1}


@functools.lru_cache(maxsize=None)
def _tables(pname):
    return mr.tables(ob.get_preset(pname))


def _encode(form, pname, C, gts, cls, match):
    """(vec [b, A, C+5] f32, match [b, A] int32) as numpy, through one of the three _ex entry points."""
    import torch
    preset = su.get_preset_by_name(pname)
    b, A = len(gts), preset.num_anchors
    if form == 'host':
        return su.encode_labels_batch(preset, C, gts, cls, match=match, return_match=True)
    if form == 'dev':
        vec, mt = su.encode_labels_batch_dev(preset, C, gts, cls, match=match, return_match=True)
        return vec.cpu().numpy(), mt.cpu().numpy()
    gt, gcls, offs = su._pack_gt(gts, cls)
    dev = torch.device('cuda', _lib.device())
    ntot = int(gcls.shape[0])
    d_gt = torch.from_numpy(gt if ntot else np.zeros((1, 4))).to(dev)
    d_cls = torch.from_numpy(gcls if ntot else np.zeros(1, np.int32)).to(dev)
    d_off = torch.from_numpy(offs).to(dev)
    ws_bytes = lib.ssd_encode_labels_ws_bytes_ex(ntot, b, RULES[match])
    assert ws_bytes > 0
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    vec = torch.empty((b, A, C + 5), dtype=torch.float32, device=dev)
    mt = torch.empty((b, A), dtype=torch.int32, device=dev)
    check(lib.ssd_encode_labels_resident_ex(pname.encode(), C, _lib.device(), d_gt.data_ptr(), d_cls.data_ptr(), d_off.data_ptr(), b, ntot,
                                            vec.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream, RULES[match], mt.data_ptr()))
    torch.cuda.synchronize()
    return vec.cpu().numpy(), mt.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _batch(name):
    """(preset name, classes, boxes per image, classes per image) of a named batch, and the oracle's answers under both rules."""
    if name == 'hand':
        pname, C = 'vgg300', 20
        gts = [np.array(boxes, np.float64).reshape(-1, 4) for _, boxes, _ in HAND_CASES]
        cls = [(np.arange(len(g)) * 3 % C).astype(np.int32) for g in gts]
    elif name in ('random_vgg300', 'random_vgg512', 'random_c127'):
        pname = 'vgg512' if name == 'random_vgg512' else 'vgg300'
        C = 127 if name == 'random_c127' else 20
        # small boxes (most have no anchor above 0.5) and mid-sized ones, 16 images, one of them empty
        rng = np.random.default_rng(7)
        sets = mr.random_boxes(rng, 0.02, 0.08, images=8, num_classes=C) + mr.random_boxes(rng, 0.05, 0.6, images=7, num_classes=C)
        sets.insert(5, (np.zeros((0, 4)), np.zeros(0, np.int32)))
        gts, cls = [s[0] for s in sets], [s[1] for s in sets]
    elif name == 'crowd100':
        # 100 small boxes in a tenth of the image: shared best anchors (rescans), exact ties, boxes past the LDS-held ones
        pname, C = 'vgg300', 20
        rng = np.random.default_rng(11)
        g = np.stack([rng.uniform(0.3, 0.4, 100), rng.uniform(0.3, 0.4, 100), rng.uniform(0.02, 0.05, 100), rng.uniform(0.02, 0.05, 100)], 1)
        gts, cls = [g], [rng.integers(0, C, 100).astype(np.int32)]
    elif name == 'identical40':
        pname, C = 'vgg300', 20
        gts, cls = [np.tile(np.array([[0.5, 0.5, 0.3, 0.3]]), (40, 1))], [(np.arange(40) % C).astype(np.int32)]
    else:
        raise KeyError(name)
    anch, aabs = _tables(pname)
    want = {rule: [mr.match_labels(g, c, ob.get_preset(pname), C, rule, anch, aabs) for g, c in zip(gts, cls)] for rule in RULES}
    return pname, C, gts, cls, want


BATCHES = ['hand', 'random_vgg300', 'random_vgg512', 'random_c127', 'crowd100', 'identical40']


def _check(got, want, C, what):
    vec, mt = got
    assert vec.dtype == np.float32 and mt.dtype == np.int32
    for i, (wvec, wmt) in enumerate(want):
        assert np.array_equal(mt[i], wmt), f'{what}, image {i}: matching'
        assert np.array_equal(vec[i][:, :C + 1], wvec[:, :C + 1]), f'{what}, image {i}: class columns'
        assert np.allclose(vec[i][:, C + 1:], wvec[:, C + 1:], rtol=2e-7, atol=1e-7), f'{what}, image {i}: offsets'


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('name', BATCHES)
def test_paper_equals_oracle(name, form):
    pname, C, gts, cls, want = _batch(name)
    _check(_encode(form, pname, C, gts, cls, 'paper'), want['paper'], C, f'{name}/{form}/paper')


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('name', ['hand', 'random_vgg300', 'random_c127'])
def test_reference_match_out_equals_oracle(name, form):
    pname, C, gts, cls, want = _batch(name)
    _check(_encode(form, pname, C, gts, cls, 'reference'), want['reference'], C, f'{name}/{form}/reference')


def test_batches_are_not_trivial():
    """The rules differ on these inputs, stage 1 has conflicts to resolve, and the workspace-held boxes are reached."""
    for name in BATCHES:
        _, _, gts, _, want = _batch(name)
        assert any(not np.array_equal(p[1], r[1]) for p, r in zip(want['paper'], want['reference'])), name
    assert _batch('crowd100')[2][0].shape[0] > 32 and _batch('identical40')[2][0].shape[0] > 32


@pytest.mark.parametrize('name', ['hand', 'random_vgg300', 'random_vgg512', 'random_c127'])
def test_match_zero_is_the_old_entry_points(name):
    """match = 0 through the _ex forms == ssd_encode_labels / _dev / _resident on the same batch, byte for byte."""
    import torch
    pname, C, gts, cls, _ = _batch(name)
    preset = su.get_preset_by_name(pname)
    old = su.encode_labels_batch(preset, C, gts, cls)
    assert np.array_equal(old, su.encode_labels_batch_dev(preset, C, gts, cls).cpu().numpy())
    # the old resident form
    gt, gcls, offs = su._pack_gt(gts, cls)
    dev = torch.device('cuda', _lib.device())
    ntot, b = int(gcls.shape[0]), len(gts)
    d = [torch.from_numpy(a).to(dev) for a in (gt, gcls, offs)]
    ws = torch.empty((lib.ssd_encode_labels_ws_bytes(ntot),), dtype=torch.uint8, device=dev)
    vec = torch.empty((b, preset.num_anchors, C + 5), dtype=torch.float32, device=dev)
    check(lib.ssd_encode_labels_resident(pname.encode(), C, _lib.device(), d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), b, ntot,
                                         vec.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert vec.cpu().numpy().tobytes() == old.tobytes()
    for form in FORMS:
        got, _ = _encode(form, pname, C, gts, cls, 'reference')
        assert got.tobytes() == old.tobytes(), form


@pytest.mark.parametrize('name', ['random_vgg300', 'crowd100', 'identical40'])
def test_paper_is_deterministic(name):
    pname, C, gts, cls, _ = _batch(name)
    for form in FORMS:
        v1, m1 = _encode(form, pname, C, gts, cls, 'paper')
        v2, m2 = _encode(form, pname, C, gts, cls, 'paper')
        assert v1.tobytes() == v2.tobytes() and m1.tobytes() == m2.tobytes(), form


def test_return_match_is_optional_and_bad_rule_raises():
    pname, C, gts, cls, _ = _batch('hand')
    preset = su.get_preset_by_name(pname)
    vec, mt = su.encode_labels_batch(preset, C, gts, cls, match='paper', return_match=True)
    assert np.array_equal(su.encode_labels_batch(preset, C, gts, cls, match='paper'), vec)
    assert np.array_equal(su.encode_labels_batch_dev(preset, C, gts, cls, match='paper').cpu().numpy(), vec)
    assert np.array_equal(mt >= 0, vec[:, :, C] == 0)
    with pytest.raises(ValueError, match='match'):
        su.encode_labels_batch(preset, C, gts, cls, match='caffe')


@pytest.mark.parametrize('workers', [0, 2])
def test_training_data_uses_the_rule(workers):
    """TrainingData(match='paper'): the labels of a batch are encode_labels_batch(match='paper') of the boxes it returns,
    through _labels (no workers) and through the feeder's resident call (workers)."""
    from ssd_tensorflow_amd.training_data import TrainingData, _gt_arrays
    td = TrainingData(None, 'vgg300', num_train=8, num_valid=4, match='paper')
    try:
        seen = 0
        for x, y, gt in td.train_generator(4, workers):
            bxs, cls = _gt_arrays(gt)
            want = su.encode_labels_batch(td.preset, td.num_classes, bxs, cls, match='paper')
            got = y.cpu().numpy() if hasattr(y, 'cpu') else np.asarray(y)
            assert got.tobytes() == want.tobytes()
            seen += 1
        assert seen == 2
    finally:
        td.close()
