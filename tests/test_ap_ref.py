"""CPU: the float64 oracle of the three AP protocols (tests/ap_ref.py) -- pinned to the oracle of the reference's protocol, the
hand-worked difficult-object case, the protocol edges; the <difficult> flag from the VOC reader through the transforms; the C
ABI of the new entry points."""
import os
import pickle
import re

import numpy as np
import pytest

import ap_ref as R
from golden_util import load
from oracle import average_precision as oap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def as_args(s):
    return (s['det_box'], s['det_conf'], s['det_cls'], s['det_sample'], s['gt_box'], s['gt_cls'], s['gt_sample'])


# ---------------------------------------------------------------------------------------------- pinning
def check_against_pinned(args, ncls):
    want = oap.compute_aps(*args)
    ap, present = R.compute(*args, ncls=ncls, protocol=R.REFERENCE)
    assert sorted(np.nonzero(present)[0]) == sorted(want)
    for k, v in want.items():
        assert ap[0, k] == v, (k, ap[0, k], v)
    slow, _ = R.compute(*args, ncls=ncls, protocol=R.REFERENCE, slow_eleven=True)      # the one-pass 11-point form is the plain one
    assert np.array_equal(slow, ap)


def test_reference_protocol_is_the_pinned_oracle_on_g8():
    g = load('g8_average_precision.npz')
    for c in range(int(g['ncases'][0])):
        args = tuple(g[f'{n}_{c}'] for n in ('det_box', 'det_conf', 'det_cls', 'det_sample', 'gt_box', 'gt_cls', 'gt_sample'))
        check_against_pinned(args, 20)
        ap, present = R.compute(*args, ncls=20)
        assert np.array_equal(ap[0, g[f'ap_cls_{c}']], g[f'ap_{c}'])


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_reference_protocol_is_the_pinned_oracle_on_random_sets(seed):
    s = R.random_set(np.random.default_rng(seed), 60, 7, dup_gt=True, empty_classes=(3,))
    check_against_pinned(as_args(s), 7)


# ---------------------------------------------------------------------------------------------- the worked case
A = [100, 200, 100, 200]
D = [500, 600, 500, 600]
NOTHING = [800, 850, 10, 60]


def worked(det_boxes, confs, protocol, flags=(0, 1)):
    n = len(confs)
    ap, present = R.compute(np.array(det_boxes, np.float32), np.array(confs, np.float32), [0] * n, [0] * n, np.array([A, D], np.float64), [0, 0],
                            [0, 0], gt_flags=list(flags), ncls=1, protocol=protocol)
    return float(ap[0, 0]), int(present[0])


def test_worked_case():
    """One class, one image, a normal box A and a difficult box D; detections 0.9 on D (IoU 1), 0.8 on nothing, 0.7 on A."""
    dets, confs = [D, NOTHING, A], [0.9, 0.8, 0.7]
    # reference: both boxes count, tp tp... D matches (tp), nothing (fp), A (tp): recall .5 .5 1, precision 1 .5 2/3
    assert worked(dets, confs, R.REFERENCE) == ((6 + 5 * (2 / 3)) / 11, 1)
    assert abs(worked(dets, confs, R.REFERENCE)[0] - 0.848485) < 1e-6
    # devkit: the detection on D is dropped; fp, then tp: one point (recall 1, precision 1/2) after the false positive's (0, 0)
    assert worked(dets, confs, R.VOC07) == (0.5, 1)
    assert worked(dets, confs, R.VOC12) == (0.5, 1)


def test_second_detection_on_a_difficult_box_is_dropped_too():
    dets, confs = [D, D, A], [0.9, 0.8, 0.7]
    assert worked(dets, confs, R.VOC07) == (1.0, 1)        # neither detection on D is a false positive
    assert worked(dets, confs, R.VOC12) == (1.0, 1)
    assert worked(dets, confs, R.REFERENCE)[0] < 1.0       # the reference's protocol: the second one is


def test_class_with_only_flagged_boxes_is_not_present():
    dets, confs = [D, A], [0.9, 0.7]
    for protocol in (R.VOC07, R.VOC12):
        assert worked(dets, confs, protocol, flags=(1, 1)) == (0.0, 0)
    assert worked(dets, confs, R.REFERENCE, flags=(1, 1)) == (1.0, 1)


@pytest.mark.parametrize('seed', [3, 4, 5])
def test_voc07_without_flags_is_the_reference_protocol(seed):
    """The reference's running maxima are the devkit's maximum over recall >= t."""
    s = R.random_set(np.random.default_rng(seed), 80, 9, ties=seed == 4, dup_gt=True, empty_classes=(2,))
    ref = R.compute(*as_args(s), ncls=9, protocol=R.REFERENCE, minoverlaps=(0.5, 0.75))
    v07 = R.compute(*as_args(s), gt_flags=np.zeros(len(s['gt_cls']), np.uint8), ncls=9, protocol=R.VOC07, minoverlaps=(0.5, 0.75))
    assert np.array_equal(ref[0], v07[0]) and np.array_equal(ref[1], v07[1])
    v12 = R.compute(*as_args(s), ncls=9, protocol=R.VOC12, minoverlaps=(0.5, 0.75))
    assert np.array_equal(ref[1], v12[1]) and not np.array_equal(ref[0], v12[0])
    assert ref[0][1].sum() < ref[0][0].sum()               # a stricter threshold costs AP


def test_flags_change_the_devkit_protocols_only():
    s = R.random_set(np.random.default_rng(11), 80, 6, flag_rate=0.3, flagged_only=(4,))
    plain = R.compute(*as_args(s), ncls=6, protocol=R.REFERENCE)
    flagged = R.compute(*as_args(s), gt_flags=s['gt_flags'], ncls=6, protocol=R.REFERENCE)
    assert np.array_equal(plain[0], flagged[0]) and plain[1][4] == 1
    for protocol in (R.VOC07, R.VOC12):
        ap, present = R.compute(*as_args(s), gt_flags=s['gt_flags'], ncls=6, protocol=protocol)
        assert present[4] == 0 and ap[0, 4] == 0.0 and present.sum() == 5
        assert not np.array_equal(ap, plain[0])


# ---------------------------------------------------------------------------------------------- the flag's way
VOC_XML = """<annotation><folder>VOC2007</folder><filename>{name}.jpg</filename>
<size><width>500</width><height>375</height><depth>3</depth></size>
<object><name>person</name><difficult>{d0}</difficult><bndbox><xmin>48</xmin><ymin>240</ymin><xmax>195</xmax><ymax>371</ymax></bndbox></object>
<object><name>horse</name><bndbox><xmin>8</xmin><ymin>12</ymin><xmax>352</xmax><ymax>298</ymax></bndbox></object>
<object><name>dog</name><difficult>{d2}</difficult><bndbox><xmin>300</xmin><ymin>100</ymin><xmax>420</xmax><ymax>200</ymax></bndbox></object>
</annotation>"""


def test_voc_source_reads_difficult(tmp_path):
    from ssd_tensorflow_amd.source_pascal_voc import PascalVOCSource
    from ssd_tensorflow_amd.utils import Box, FlaggedBox
    root = tmp_path / 'test' / 'VOCdevkit' / 'VOC2012'
    os.makedirs(root / 'Annotations'); os.makedirs(root / 'ImageSets' / 'Main'); os.makedirs(root / 'JPEGImages')
    flags = {'a': (1, 0), 'b': (0, 1), 'c': (0, 0)}
    for n, (d0, d2) in flags.items():
        (root / 'Annotations' / (n + '.xml')).write_text(VOC_XML.format(name=n, d0=d0, d2=d2))
    (root / 'ImageSets' / 'Main' / 'test.txt').write_text('\n'.join(flags) + '\n')
    src = PascalVOCSource()
    src.load_test_data(str(tmp_path), require_image=False)
    assert src.num_test == 3
    got = {os.path.basename(s.filename)[0]: [bool(getattr(b, 'difficult', False)) for b in s.boxes] for s in src.test_samples}
    assert got == {'a': [True, False, False], 'b': [False, False, True], 'c': [False, False, False]}
    # an unflagged object stays the reference's plain record; a flagged one is still that record to every consumer
    a = {os.path.basename(s.filename)[0]: s for s in src.test_samples}['a']
    assert type(a.boxes[1]) is Box and isinstance(a.boxes[0], FlaggedBox) and isinstance(a.boxes[0], Box)
    assert a.boxes[0] == Box(*a.boxes[0]) and len(a.boxes[0]) == 4


def test_flagged_box_is_a_box():
    from ssd_tensorflow_amd.utils import Box, FlaggedBox, Point, Size, normalize_box
    b = Box('dog', 11, Point(0.5, 0.25), Size(0.2, 0.1))
    f = FlaggedBox('dog', 11, Point(0.5, 0.25), Size(0.2, 0.1), True)
    assert b == f and f == b and hash(b) == hash(f) and tuple(f) == tuple(b) and len({b, f}) == 1
    assert f.difficult is True and FlaggedBox(*b).difficult is False and not hasattr(b, 'difficult')
    label, labelid, center, size = f
    assert (label, labelid, center, size) == tuple(b) and f.center.x == 0.5
    g = pickle.loads(pickle.dumps(f))
    assert g == f and type(g) is FlaggedBox and g.difficult is True
    assert pickle.loads(pickle.dumps(FlaggedBox(*b))).difficult is False
    assert f._replace(label='cat').difficult is True and f._replace(label='cat').label == 'cat'
    assert normalize_box(f).difficult is True and normalize_box(f) == normalize_box(b) and type(normalize_box(b)) is Box


def test_flag_survives_flip_and_crop():
    from ssd_tensorflow_amd import transforms as T
    from ssd_tensorflow_amd.utils import Box, FlaggedBox, Point, Sample, Size
    size = Size(200, 100)
    boxes = [FlaggedBox('dog', 11, Point(0.3, 0.5), Size(0.2, 0.4), True), Box('cat', 7, Point(0.6, 0.5), Size(0.2, 0.4)),
             FlaggedBox('cow', 9, Point(0.7, 0.4), Size(0.1, 0.2), False)]
    gt = Sample('x', boxes, size)
    plan = T.ImagePlan(np.zeros((size.h, size.w, 3), np.uint8))
    _, _, flipped = T.HorizontalFlipTransform()(plan, None, gt)
    assert [getattr(b, 'difficult', False) for b in flipped.boxes] == [True, False, False]
    assert flipped.boxes[0] == Box('dog', 11, Point(1 - 0.3, 0.5), Size(0.2, 0.4))
    _, _, cropped = T.SamplerTransform(sample=True).crop(plan, None, gt, [20, 180, 10, 90])
    assert [b.label for b in cropped.boxes] == ['dog', 'cat', 'cow']
    assert [getattr(b, 'difficult', False) for b in cropped.boxes] == [True, False, False]
    assert cropped.boxes[0] == T.transform_box(Box(*boxes[0]), size, Size(160, 80), -10, -20)
    _, _, both = T.HorizontalFlipTransform()(*T.SamplerTransform(sample=True).crop(plan, None, gt, [20, 180, 10, 90]))
    assert [getattr(b, 'difficult', False) for b in both.boxes] == [True, False, False]


# ---------------------------------------------------------------------------------------------- ABI
NEW_SYMBOLS = ('ssd_average_precision_ex', 'ssd_ap_create', 'ssd_ap_destroy', 'ssd_ap_clear', 'ssd_ap_add_dev', 'ssd_ap_add_host',
               'ssd_ap_count', 'ssd_ap_fetch', 'ssd_ap_compute')


def test_abi_of_the_ap_entry_points():
    import ctypes as C
    from ssd_tensorflow_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'ssdvgg_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for name in NEW_SYMBOLS:
        assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES, name
        m = re.search(r'\bint\s+%s\s*\(([^;]*?)\)\s*;' % name, code, flags=re.S)
        assert m, name + ' is not declared'
        params = [p for p in m.group(1).split(',') if p.strip()]
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == len(params), (name, len(args), len(params))
        for p, a in zip(params, args):                              # pointers are pointers, scalars the scalar the header names
            if '*' in p or 'ssd_ap_accumulator' in p:
                assert a is C.c_void_p or issubclass(a, C._Pointer), (name, p)
            elif 'long long' in p:
                assert a is C.c_longlong, (name, p)
            elif 'double' in p:
                assert a is C.c_double, (name, p)
            else:
                assert a is C.c_int, (name, p)
    assert re.search(r'SSD_AP_REFERENCE\s*=\s*0\s*,\s*SSD_AP_VOC07\s*=\s*1\s*,\s*SSD_AP_VOC12\s*=\s*2', code)
    # the old entry keeps its place and its signature
    assert _lib.SIGNATURES['ssd_average_precision'][1][11] is C.c_double and len(_lib.SIGNATURES['ssd_average_precision'][1]) == 14


def test_protocol_and_threshold_arguments_are_checked_on_the_host():
    from ssd_tensorflow_amd import average_precision as apm
    assert apm.PROTOCOLS == {'reference': 0, 'voc07': 1, 'voc12': 2}
    with pytest.raises(ValueError):
        apm.APCalculator(protocol='coco')
    with pytest.raises(ValueError):
        apm.APCalculator(minoverlap=[0.5] * 11)
    calc = apm.APCalculator(minoverlap=[0.5, 0.75], protocol='voc12')
    assert calc.compute_aps() == {} and calc.protocol == 'voc12'
