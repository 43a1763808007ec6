"""-m gpu: DetectionOutput through the C ABI against the numpy oracle tests/detout_ref.py: count, confidence
bits, class, anchor and box of every image compared with np.array_equal, no tolerance.  The cases (tests/detout_cases.py) are
built and their expected results computed once per process; tests/test_detout_ref.py shows what each case is able to see."""
import ctypes as C

import numpy as np
import pytest
import torch

import detout_cases as dc
import detout_ref as dr
from gpu_util import dev as _dev, host
from ssd_tensorflow_amd import _lib
from ssd_tensorflow_amd import average_precision as apm
from ssd_tensorflow_amd import ssdutils as su
from ssd_tensorflow_amd._lib import lib, last_error, np_ptr

pytestmark = pytest.mark.gpu


def dev(a):
    """a device copy (the cases' arrays are read-only; torch wants a writable source)"""
    return _dev(np.array(a))


def host_entry(pname, pred, thr, k, keep, out_cap):
    b, A, nv = pred.shape
    count = np.full(b, -1, np.int32)
    conf = np.full((b, out_cap), -1, np.float32)
    cls = np.full((b, out_cap), -1, np.int32)
    idx = np.full((b, out_cap), -1, np.int32)
    box = np.full((b, out_cap, 4), -1, np.int32)
    rc = lib.ssd_detection_output(pname.encode(), nv - 5, 0, np_ptr(pred), b, thr, k, keep, out_cap, np_ptr(count), np_ptr(conf),
                                  np_ptr(cls), np_ptr(idx), np_ptr(box))
    assert rc == 0, last_error()
    return count, conf, cls, idx, box


_ANCHORS_DEV = {}


def anchors_dev(pname):
    if pname not in _ANCHORS_DEV:
        _ANCHORS_DEV[pname] = dev(su.anchors_array(pname))
    return _ANCHORS_DEV[pname]


def dev_entry(pname, pred, thr, k, keep, out_cap, ws_short=0, pred_dev=None):
    """-> (rc, outputs); the outputs start as -1 everywhere, so a row the pass did not write shows"""
    b, A, nv = pred.shape
    need = lib.ssd_detection_output_ws_bytes(pname.encode(), nv - 5, b, k)
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device='cuda:0')
    d_pred = dev(pred) if pred_dev is None else pred_dev
    count = torch.full((b,), -1, dtype=torch.int32, device='cuda:0')
    conf = torch.full((b, out_cap), -1, dtype=torch.float32, device='cuda:0')
    cls = torch.full((b, out_cap), -1, dtype=torch.int32, device='cuda:0')
    idx = torch.full((b, out_cap), -1, dtype=torch.int32, device='cuda:0')
    box = torch.full((b, out_cap, 4), -1, dtype=torch.int32, device='cuda:0')
    torch.cuda.synchronize()
    rc = lib.ssd_detection_output_dev(pname.encode(), nv - 5, anchors_dev(pname).data_ptr(), d_pred.data_ptr(), b, thr, k, keep, out_cap,
                                      count.data_ptr(), conf.data_ptr(), cls.data_ptr(), idx.data_ptr(), box.data_ptr(), ws.data_ptr(),
                                      need - ws_short, torch.cuda.current_stream().cuda_stream)
    return rc, tuple(host(t) for t in (count, conf, cls, idx, box))


def check_against(want, outs, out_cap, untouched=None):
    count, conf, cls, idx, box = outs
    for i, w in enumerate(want):
        n = len(w['idx'])
        assert count[i] == n, f'image {i}: count {count[i]} != {n}'
        m = min(n, out_cap)
        assert np.array_equal(conf[i, :m].view(np.uint32), w['conf'][:m].view(np.uint32)), f'image {i}: confidences'
        assert np.array_equal(cls[i, :m], w['cls'][:m]), f'image {i}: classes'
        assert np.array_equal(idx[i, :m], w['idx'][:m]), f'image {i}: anchors'
        assert np.array_equal(box[i, :m], w['box'][:m]), f'image {i}: boxes'
        if untouched is not None:       # rows past the count: zero from the host entry, not written by the device entry
            assert (conf[i, m:] == untouched).all() and (cls[i, m:] == untouched).all() and (idx[i, m:] == untouched).all()
            assert (box[i, m:] == untouched).all()


@pytest.mark.parametrize('name', dc.NAMES)
def test_host_entry_equals_the_oracle(name):
    pname, pred, thr, k, keep = dc.case(name)
    before = pred.copy()
    outs = host_entry(pname, pred, thr, k, keep, keep)
    assert np.array_equal(pred, before), 'pred must not be modified'
    check_against(dc.expected(name), outs, keep, untouched=0)


@pytest.mark.parametrize('name', dc.NAMES)
def test_dev_entry_equals_the_oracle(name):
    pname, pred, thr, k, keep = dc.case(name)
    d_pred = dev(pred)
    rc, outs = dev_entry(pname, pred, thr, k, keep, keep, pred_dev=d_pred)
    assert rc == 0, last_error()
    assert np.array_equal(host(d_pred), pred), 'pred must not be modified'
    check_against(dc.expected(name), outs, keep, untouched=-1)


def test_the_result_is_deterministic():
    pname, pred, thr, k, keep = dc.case('softmax-C28')
    first = dev_entry(pname, pred, thr, k, keep, keep)[1]
    for _ in range(2):
        again = dev_entry(pname, pred, thr, k, keep, keep)[1]
        assert all(np.array_equal(a.view(np.int32), f.view(np.int32)) for a, f in zip(again, first))


@pytest.mark.parametrize('entry', ['host', 'dev'])
def test_out_cap_below_the_count_clips_rows(entry):
    pname, pred, thr, k, keep = dc.case('softmax-C3')
    want = dc.expected('softmax-C3')
    assert min(len(w['idx']) for w in want) > 50
    if entry == 'host':
        outs = host_entry(pname, pred, thr, k, keep, 50)
    else:
        rc, outs = dev_entry(pname, pred, thr, k, keep, 50)
        assert rc == 0, last_error()
    assert outs[1].shape == (3, 50)
    check_against(want, outs, 50)


def test_one_class_equals_the_argmax_path_byte_for_byte():
    pname, pred, thr, k, keep = dc.case('one-class')
    b = pred.shape[0]
    outs = host_entry(pname, pred, thr, k, keep, keep)
    count = np.zeros(b, np.int32); conf = np.zeros((b, keep), np.float32); cls = np.zeros((b, keep), np.int32)
    idx = np.zeros((b, keep), np.int32); box = np.zeros((b, keep, 4), np.int32)
    rc = lib.ssd_decode_nms(pname.encode(), 1, 0, np_ptr(pred), b, thr, -1, keep, keep, 1, np_ptr(count), np_ptr(conf), np_ptr(cls),
                            np_ptr(idx), np_ptr(box))
    assert rc == 0, last_error()
    assert np.array_equal(outs[0], count) and count.min() > 50
    for i in range(b):
        n = count[i]
        for got, want in zip(outs[1:], (conf, cls, idx, box)):
            assert got[i, :n].tobytes() == want[i, :n].tobytes()


def test_python_mirror_returns_the_reference_lists():
    pname, pred, thr, k, keep = dc.case('sparse')
    preset = su.get_preset_by_name(pname)
    want = dc.expected('sparse')[2]
    names = {0: 'a', 1: 'b', 2: 'c'}
    for arg in (preset, pname, [None] * preset.num_anchors):
        boxes = su.detection_output(pred[2], arg, thr, names, k, keep)
        assert len(boxes) == len(want['idx'])
        assert [float(c) for c, _ in boxes] == [float(c) for c in want['conf']]
        assert [b.labelid for _, b in boxes] == want['cls'].tolist() and boxes[0][1].label == names[int(want['cls'][0])]
    ref = su.boxes_from_detection({k2: v for k2, v in want.items()}, names)
    assert [(b.center, b.size) for _, b in boxes] == [(b.center, b.size) for _, b in ref]


REFUSED = [  # (what, preset, C, b, thr, k, keep, out_cap, ws bytes short)
    ('unknown preset', 'vgg999', 3, 1, 0.01, 400, 200, 200, 0),
    ('no classes', 'vgg300', 0, 1, 0.01, 400, 200, 200, 0),
    ('128 classes', 'vgg300', 128, 1, 0.01, 400, 200, 200, 0),
    ('batch 0', 'vgg300', 3, 0, 0.01, 400, 200, 200, 0),
    ('batch 4097', 'vgg300', 3, 4097, 0.01, 400, 200, 200, 0),
    ('negative threshold', 'vgg300', 3, 1, -0.5, 400, 200, 200, 0),
    ('nan threshold', 'vgg300', 3, 1, float('nan'), 400, 200, 200, 0),
    ('infinite threshold', 'vgg300', 3, 1, float('inf'), 400, 200, 200, 0),
    ('nms_top_k 0', 'vgg300', 3, 1, 0.01, 0, 200, 200, 0),
    ('nms_top_k 1025', 'vgg300', 3, 1, 0.01, 1025, 200, 200, 0),
    ('keep_top_k 0', 'vgg300', 3, 1, 0.01, 400, 0, 200, 0),
    ('keep_top_k 1025', 'vgg300', 3, 1, 0.01, 400, 1025, 200, 0),
    ('out_cap 0', 'vgg300', 3, 1, 0.01, 400, 200, 0, 0),
    ('workspace one byte short', 'vgg300', 3, 1, 0.01, 400, 200, 200, 1),
]


@pytest.mark.parametrize('case', REFUSED, ids=[c[0] for c in REFUSED])
def test_refused_arguments_launch_nothing(case):
    what, pname, ncls, b, thr, k, keep, out_cap, short = case
    # valid buffers of a 3-class, 1-image pass whatever is asked for: a launch that did happen would write into them
    _, pred, _, _, _ = dc.case('softmax-C3')
    d_pred = dev(pred[:1])
    ws = torch.empty(lib.ssd_detection_output_ws_bytes(b'vgg300', 3, 1, 1024), dtype=torch.uint8, device='cuda:0')
    need = lib.ssd_detection_output_ws_bytes(b'vgg300', 3, 1, 400)
    outs = [torch.full((n,), -1, dtype=torch.int32, device='cuda:0') for n in (8, 1024, 1024, 1024, 4096)]
    torch.cuda.synchronize()
    rc = lib.ssd_detection_output_dev(pname.encode(), ncls, anchors_dev('vgg300').data_ptr(), d_pred.data_ptr(), b, thr, k, keep,
                                      out_cap, *[t.data_ptr() for t in outs], ws.data_ptr(), (need - 1) if short else ws.numel(),
                                      torch.cuda.current_stream().cuda_stream)
    assert rc != 0 and last_error(), what
    assert all((host(t) == -1).all() for t in outs), what + ': an output was written'
    if not short:       # the host entry refuses the same arguments
        z = np.zeros(4096, np.int32)
        assert lib.ssd_detection_output(pname.encode(), ncls, 0, np_ptr(pred[:1]), b, thr, k, keep, out_cap, np_ptr(z), np_ptr(z.view(np.float32)),
                                        np_ptr(z), np_ptr(z), np_ptr(z)) != 0, what
        assert not z.any()


def test_null_pointers_are_refused():
    assert lib.ssd_detection_output_dev(b'vgg300', 3, None, None, 1, 0.01, 400, 200, 200, None, None, None, None, None, None, 1 << 30, None) != 0
    assert 'null' in last_error()


# ------------------------------------------------------------------------------------- through a handle
def test_handle_detect_last_all_and_the_device_accumulator():
    from ssd_tensorflow_amd.ssdvgg import SSDVGG, Session
    from ssd_tensorflow_amd.utils import Box, Size, abs2prop
    ncls, b = 3, 2
    names = {i: 'class_%d' % i for i in range(ncls)}
    rng = np.random.default_rng(8)
    anch = dc.anchors('vgg300')
    with Session(0) as sess:
        net = SSDVGG(sess, 'vgg300')
        net.build_from_vgg(None, ncls, max_batch=b, training=False, seed=7)
        x = torch.from_numpy(rng.integers(0, 256, (b, 300, 300, 3)).astype(np.float32)).cuda()
        net.infer_dev(x)
        pred = net._dev_result(b, True)
        dets = net.detect_last(b, 0.01, decode='all')
        argmax = net.detect_last(b, 0.01, None, 200)
        for i in range(b):
            want = dr.detection_output(pred[i], anch, 0.01, 400, 200)
            assert len(want['idx']) > 20
            got = {k: v.astype(np.int64) if k != 'conf' else v for k, v in dets[i].items()}
            assert dr.same(got, want), f'image {i}'
            # the default (decode='argmax') still runs the reference decode
            ref = ob_detect(pred[i], anch)
            assert np.array_equal(argmax[i]['idx'], ref['idx']) and np.array_equal(argmax[i]['box'], ref['box'])
        small = net.detect_last(b, 0.01, decode='all', nms_top_k=5, keep_top_k=7)
        for i in range(b):
            want = dr.detection_output(pred[i], anch, 0.01, 5, 7)
            assert dr.same({k: v.astype(np.int64) if k != 'conf' else v for k, v in small[i].items()}, want)
        for bad in (dict(detections_cap=100), dict(max_out=50), dict(nms=False)):
            with pytest.raises(ValueError, match="decode='all'"):
                net.detect_last_launch(b, 0.01, decode='all', **bad)
        with pytest.raises(ValueError, match='argmax'):
            net.detect_last_launch(b, 0.01, decode='both')
        with pytest.raises(RuntimeError, match='nms_top_k'):
            net.detect_last_launch(b, 0.01, decode='all', nms_top_k=2000)
        # the device accumulator fed from the pass's slots against the host calculator fed the fetched lists
        gts = []
        for _ in range(b):
            gt = []
            for _ in range(3):
                x0, y0 = (int(v) for v in rng.integers(0, 600, 2)); w, h = (int(v) for v in rng.integers(100, 400, 2))
                c = int(rng.integers(0, ncls))
                gt.append(Box(names[c], c, *abs2prop(x0, x0 + w, y0, y0 + h, Size(1000, 1000))))
            gts.append(gt)
        calc = apm.DeviceAPCalculator(0, ncls)
        hostc = apm.APCalculator()
        ticket = net.detect_last_launch(b, 0.01, decode='all')
        calc.add_pass(ticket, gts)
        n = 0
        for gt, det in zip(gts, ticket.get()):
            hostc.add_detections(gt, su.boxes_from_detection(det, names)); n += len(det['conf'])
        want = hostc.compute_aps()
        assert list(calc.compute_aps().items()) == list(want.items()) and len(want) >= 1
        assert calc.num_detections() == n > 40
        calc.close()


def ob_detect(pred, anch):
    from oracle import boxes as ob
    return ob.detect(pred, anch, 0.01, None, 200)
