"""More than 27 classes without a GPU: the oracle against the reference-pinned 80-class fixtures (g11 / g12), the
synthetic data sets at N classes, the class names a checkpoint stores and infer.py resolves."""
import numpy as np
import pytest

from oracle import boxes as ob
from golden_util import load
from ssd_tensorflow_amd.infer import resolve_class_names
from ssd_tensorflow_amd.training_data import TrainingData, VOC_NAMES, default_class_names

PRESETS = ['vgg300', 'vgg512']


@pytest.mark.parametrize('pname', PRESETS)
def test_oracle_reproduces_g12_labels_c80(pname):
    g = load(f'g12_labels_c80_{pname}.npz')
    C = int(g['num_classes'][0])
    assert C == 80
    op = ob.get_preset(pname)
    anch = ob.anchors(op); aabs = ob.anchors_abs(anch)
    for ci in range(int(g['ncases'][0])):
        vec = ob.encode_labels(g[f'gt_{ci}'], g[f'cls_{ci}'], op, C, anch, aabs)
        assert vec.shape == (len(anch), C + 5)
        pos = np.nonzero(vec[:, C] == 0)[0]
        assert np.array_equal(pos, g[f'pos_{ci}']) and np.array_equal(vec[pos], g[f'rows_{ci}']), ci
    assert max(int(g[f'cls_{ci}'].max()) for ci in range(int(g['ncases'][0]))) == C - 1


@pytest.mark.parametrize('pname', PRESETS)
def test_oracle_reproduces_g11_detect_c80(pname):
    g = load(f'g11_detect_c80_{pname}.npz')
    A, C = int(g['A'][0]), int(g['num_classes'][0])
    oa = ob.anchors(ob.get_preset(pname))
    row = np.zeros(C + 5, np.float32); row[C] = 1
    n = 0
    for pi in range(int(g['npred'][0])):
        pred = np.tile(row, (A, 1))
        pred[g[f'predrows_{pi}']] = g[f'predvals_{pi}']
        for si in range(int(g['nset'][0])):
            tag = f'{pi}_{si}'
            thr, cap, mo = g[f'set_{tag}']
            cap = None if cap < 0 else int(cap)
            mo = None if mo < 0 else int(mo)
            det = ob.decode(pred, oa, float(thr), cap)
            for k in ('idx', 'cls', 'conf', 'box'):
                assert np.array_equal(det[k], g[f'{k}_{tag}']), (tag, k)
            assert np.array_equal(ob.suppress(det, mo), g[f'keep_{tag}']), tag
            n += 1
    assert n == 9
    assert max(int(g[f'cls_{pi}_0'].max()) for pi in range(3)) > 27          # the wide class ids are exercised


def test_synthetic_data_with_80_classes():
    td = TrainingData(None, 'vgg300', num_train=64, num_valid=4, device_tensors=False, synthetic_classes=80)
    try:
        assert td.num_classes == 80 and len(td.lid2name) == 80 and td.lid2name[79] == 'class_79'
        ids = [b.labelid for i in range(64) for b in td._sample(i, 0)[1]]
        assert min(ids) >= 0 and max(ids) <= 79 and max(ids) > 27
        gt = td._sample(0, 0)[1]
        op = ob.get_preset('vgg300')
        anch = ob.anchors(op)
        g = np.array([[b.center.x, b.center.y, b.size.w, b.size.h] for b in gt])
        y = ob.encode_labels(g, np.array([b.labelid for b in gt]), op, td.num_classes, anch, ob.anchors_abs(anch))
        assert y.shape == (td.preset.num_anchors, 85)
    finally:
        td.close()
    td = TrainingData('shapes', 'vgg300', num_train=8, num_valid=2, device_tensors=False, synthetic_classes=2)
    try:
        assert {b.labelid for i in range(8) for b in td._sample(i, 0)[1]} <= {0, 1}
    finally:
        td.close()


def test_synthetic_class_count_is_checked():
    with pytest.raises(RuntimeError, match='1..127'):
        TrainingData(None, 'vgg300', num_train=4, num_valid=1, device_tensors=False, synthetic_classes=128)


def test_default_class_names():
    assert TrainingData(None, 'vgg300', num_train=4, num_valid=1, device_tensors=False).lid2name == dict(enumerate(VOC_NAMES))
    assert default_class_names(20) == list(VOC_NAMES)
    assert default_class_names(3) == ['class_0', 'class_1', 'class_2']


def test_infer_class_name_resolution():
    # names stored in the checkpoint (a unicode array) are used when no data source names the classes
    stored = np.array(['cat', 'dog', 'zebra'], dtype=np.str_)
    assert resolve_class_names(3, None, stored) == {0: 'cat', 1: 'dog', 2: 'zebra'}
    # ... but a data source's names win
    assert resolve_class_names(3, {0: 'a', 1: 'b', 2: 'c'}, stored) == {0: 'a', 1: 'b', 2: 'c'}
    # an old 20-class checkpoint without names: the VOC names
    assert resolve_class_names(20, None, None) == dict(enumerate(VOC_NAMES))
    # an unnamed N-class checkpoint: class_<id>
    names = resolve_class_names(80, None, None)
    assert len(names) == 80 and names[0] == 'class_0' and names[79] == 'class_79'
