"""CPU: the C ABI and the Python names of the matching rules.  Nothing here touches a GPU: a bad
`match` is refused on the host before any HIP call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ssd_tensorflow_amd import _lib, ssdutils as su, transforms as T
from ssd_tensorflow_amd._lib import lib

NEW = ['ssd_encode_labels_ex', 'ssd_encode_labels_dev_ex', 'ssd_encode_labels_resident_ex', 'ssd_encode_labels_ws_bytes_ex']
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'ssdvgg_hip.h')


def test_the_new_symbols_exist():
    text = open(HEADER).read()
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert re.search(r'\b%s\(' % name, text), name
    assert re.search(r'SSD_MATCH_REFERENCE\s*=\s*0\b', text) and re.search(r'SSD_MATCH_PAPER\s*=\s*1\b', text)
    assert su.MATCH_RULES == {'reference': 0, 'paper': 1}


def test_workspace_sizes():
    for ntot in (0, 1, 7, 100, 512, 100000):
        old = (max(ntot, 1) * 7 * 4 + 64 + 255) // 256 * 256         # the value every earlier build returned
        assert lib.ssd_encode_labels_ws_bytes(ntot) == old
        assert lib.ssd_encode_labels_ws_bytes_ex(ntot, 32, 0) == old
        assert lib.ssd_encode_labels_ws_bytes_ex(ntot, 32, 1) >= old
    assert lib.ssd_encode_labels_ws_bytes_ex(8, 1, 2) == 0 and 'match' in _lib.last_error()


@pytest.mark.parametrize('bad', [-1, 2, 7])
def test_a_bad_match_is_refused_on_the_host(bad):
    gt = np.array([[0.5, 0.5, 0.3, 0.3]], np.float64)
    cls = np.zeros(1, np.int32)
    offs = np.array([0, 1], np.int32)
    vec = np.full((8732, 25), 7.0, np.float32)
    p = _lib.np_ptr
    assert lib.ssd_encode_labels_ex(b'vgg300', 20, 0, p(gt), p(cls), p(offs), 1, p(vec), bad, None) != 0
    assert 'match' in _lib.last_error()
    # the device forms look at `match` before at any pointer: the (never dereferenced) device pointers are null
    assert lib.ssd_encode_labels_dev_ex(b'vgg300', 20, 0, p(gt), p(cls), p(offs), 1, None, None, bad, None) != 0
    assert 'match' in _lib.last_error()
    assert lib.ssd_encode_labels_resident_ex(b'vgg300', 20, 0, None, None, None, 1, 1, None, None, None, bad, None) != 0
    assert 'match' in _lib.last_error()
    assert (vec == 7.0).all()


def test_rule_names_parse():
    assert su.match_id('reference') == 0 and su.match_id('paper') == 1
    preset = su.get_preset_by_name('vgg300')
    for bad in ('caffe', 'Paper', '', None, 1):
        with pytest.raises(ValueError, match='match'):
            su.match_id(bad)
        with pytest.raises(ValueError, match='match'):
            su.encode_labels_batch(preset, 20, [np.zeros((0, 4))], [np.zeros(0, np.int32)], match=bad)
        with pytest.raises(ValueError, match='match'):
            su.encode_labels_batch_dev(preset, 20, [np.zeros((0, 4))], [np.zeros(0, np.int32)], match=bad)
        with pytest.raises(ValueError, match='match'):
            T.LabelCreatorTransform(preset=preset, num_classes=20, match=bad)
    for rule in ('reference', 'paper'):
        assert T.LabelCreatorTransform(preset=preset, num_classes=20, match=rule).match == rule
        assert [t for t in T.build_train_transforms(preset, 20, 50, 0.5, match=rule) if isinstance(t, T.LabelCreatorTransform)][0].match == rule
        assert [t for t in T.build_valid_transforms(preset, 20, match=rule) if isinstance(t, T.LabelCreatorTransform)][0].match == rule
    assert T.LabelCreatorTransform(preset=preset, num_classes=20).match == 'reference'


def test_training_data_refuses_an_unknown_rule():
    from ssd_tensorflow_amd.training_data import TrainingData
    with pytest.raises(ValueError, match='match'):
        TrainingData(None, 'vgg300', num_train=4, num_valid=2, match='caffe')
    td = TrainingData(None, 'vgg300', num_train=4, num_valid=2, match='paper')
    try:
        assert td.match == 'paper'
    finally:
        td.close()
