"""-m gpu: AP on the GPU end to end -- ssd_average_precision_ex (three protocols, threshold lists) against the float64 oracle
of tests/ap_ref.py, the device accumulator behind synthetic and real detection passes against the host lists, and the drivers'
--ap-on gpu against --ap-on host.  Every comparison is == on float64."""
import functools
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import ap_ref as R
from ssd_tensorflow_amd import average_precision as apm, ssdutils as su
from ssd_tensorflow_amd._lib import lib, check, np_ptr
from ssd_tensorflow_amd.utils import Box, FlaggedBox, Size, abs2prop, prop2abs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMG = Size(1000, 1000)
THRESHOLDS = {1: (0.5,), 10: tuple(float(v) for v in np.arange(0.5, 0.96, 0.05))}
PROTOCOL_NAMES = {0: 'reference', 1: 'voc07', 2: 'voc12'}


# ------------------------------------------------------------------------------------- ssd_average_precision_ex
@functools.lru_cache(maxsize=None)
def eval_set(n_det, ncls):
    """Equal confidences, duplicate ground-truth boxes, images and classes without ground truth, a class without detections, a
    class with only flagged boxes (where the class count has room for them), flagged boxes among the others."""
    rng = np.random.default_rng(1000 * ncls + n_det)
    many = ncls >= 20
    s = R.random_set(rng, max(6, n_det // 4), ncls, n_det=n_det, flag_rate=0.2, dup_gt=True, empty_classes=(3,) if many else (),
                     flagged_only=(5,) if many else ())
    if many:
        s['det_cls'][s['det_cls'] == 7] = 8                                     # class 7: ground truth, no detection
    s['det_conf'] = (np.ceil(s['det_conf'] * 48) / 48).astype(np.float32)       # at most 48 values: ties from 49 detections on
    assert len(s['det_conf']) == n_det
    return s


@functools.lru_cache(maxsize=None)
def oracle(n_det, ncls, protocol, n_thr):
    s = eval_set(n_det, ncls)
    return R.compute(s['det_box'], s['det_conf'], s['det_cls'], s['det_sample'], s['gt_box'], s['gt_cls'], s['gt_sample'], s['gt_flags'],
                     ncls=ncls, protocol=protocol, minoverlaps=THRESHOLDS[n_thr])


def gpu_ex(s, ncls, protocol, thresholds):
    thr = np.ascontiguousarray(thresholds, np.float64)
    ap = np.full((len(thr), ncls), -1.0); present = np.full(ncls, -1, np.int32)
    check(lib.ssd_average_precision_ex(0, len(s['det_conf']), np_ptr(s['det_box']), np_ptr(s['det_conf']), np_ptr(s['det_cls']),
                                       np_ptr(s['det_sample']), len(s['gt_cls']), np_ptr(s['gt_box']), np_ptr(s['gt_cls']),
                                       np_ptr(s['gt_sample']), np_ptr(s['gt_flags']), ncls, protocol, len(thr), np_ptr(thr), np_ptr(ap),
                                       np_ptr(present)))
    return ap, present


@pytest.mark.parametrize('n_thr', [1, 10])
@pytest.mark.parametrize('ncls', [1, 20, 127])
@pytest.mark.parametrize('n_det', [0, 1, 255, 256, 257, 5000])
@pytest.mark.parametrize('protocol', [0, 1, 2])
def test_average_precision_ex_against_oracle(protocol, n_det, ncls, n_thr):
    s = eval_set(n_det, ncls)
    want_ap, want_present = oracle(n_det, ncls, protocol, n_thr)
    ap, present = gpu_ex(s, ncls, protocol, THRESHOLDS[n_thr])
    assert np.array_equal(present, want_present)
    assert np.array_equal(ap, want_ap), np.argwhere(ap != want_ap)[:5]
    if n_det == 5000:
        assert len(np.unique(s['det_conf'])) <= 48 and want_ap.max() > 0.1
        if ncls >= 20:          # the awkward classes are in the set
            assert present[3] == 0 and present[7] == 1 and present[5] == (1 if protocol == 0 else 0)
            assert not (s['det_cls'] == 7).any() and (s['det_cls'] == 3).any()


def test_old_entry_point_is_protocol_zero_with_one_threshold():
    s = eval_set(5000, 20)
    ap = np.zeros(20); present = np.zeros(20, np.int32)
    check(lib.ssd_average_precision(0, 5000, np_ptr(s['det_box']), np_ptr(s['det_conf']), np_ptr(s['det_cls']), np_ptr(s['det_sample']),
                                    len(s['gt_cls']), np_ptr(s['gt_box']), np_ptr(s['gt_cls']), np_ptr(s['gt_sample']), 20, 0.5, np_ptr(ap),
                                    np_ptr(present)))
    want_ap, want_present = oracle(5000, 20, 0, 1)
    assert np.array_equal(ap, want_ap[0]) and np.array_equal(present, want_present)


def test_ex_refusals():
    s = eval_set(255, 20)
    for protocol, thr in ((3, (0.5,)), (-1, (0.5,)), (0, ()), (0, (0.5,) * 11)):
        with pytest.raises(RuntimeError):
            gpu_ex(s, 20, protocol, thr)
    with pytest.raises(RuntimeError):
        gpu_ex(s, 128, 0, (0.5,))


# ------------------------------------------------------------------------------------- the accumulator on synthetic slots
NAMES = {k: 'c%d' % k for k in range(127)}
CHANGING = (990, 1052, 173, 481)           # prop2abs(abs2prop(.)) gives (989, 1052, 173, 481)


def roundtrip(box):
    return prop2abs(*abs2prop(int(box[0]), int(box[1]), int(box[2]), int(box[3]), IMG), IMG)


def make_passes(seed, b, out_cap, n_pass, ncls, flag_rate=0.25, bad_cls=()):
    """[(slot arrays, ground truth per image)]: counts from 0 to beyond out_cap, entries behind a count filled with rubbish"""
    rng = np.random.default_rng(seed)
    passes = []
    for p in range(n_pass):
        count = rng.integers(0, out_cap + 3, b).astype(np.int32)
        count[rng.integers(0, b)] = 0 if p % 2 else out_cap + 2
        conf = (np.ceil(rng.random((b, out_cap)) * 32) / 32).astype(np.float32)
        cls = np.full((b, out_cap), -7, np.int32)
        box = rng.integers(-2000, 2000, (b, out_cap, 4)).astype(np.int32)
        gts = []
        for i in range(b):
            gt = []
            for _ in range(int(rng.integers(0, 3))):
                x0, y0 = (int(v) for v in rng.integers(0, 700, 2)); w, h = (int(v) for v in rng.integers(30, 300, 2))
                k = int(rng.integers(0, ncls))
                center, size = abs2prop(x0, x0 + w, y0, y0 + h, IMG)
                gt.append(FlaggedBox(NAMES[k], k, center, size, True) if rng.random() < flag_rate else Box(NAMES[k], k, center, size))
            gts.append(gt)
            n = min(int(count[i]), out_cap)
            for j in range(n):
                if gt and rng.random() < 0.7:
                    g = gt[int(rng.integers(0, len(gt)))]
                    bx = np.array(prop2abs(g.center, g.size, IMG)) + rng.integers(-30, 30, 4)
                    k = g.labelid if rng.random() < 0.9 else int(rng.integers(0, ncls))
                else:
                    x0, y0 = (int(v) for v in rng.integers(-50, 900, 2))
                    bx = np.array([x0, x0 + int(rng.integers(1, 400)), y0, y0 + int(rng.integers(1, 400))])
                    k = int(rng.integers(0, ncls))
                if rng.random() < 0.1:
                    bx = np.array(CHANGING)
                box[i, j] = bx; cls[i, j] = k
            for k in bad_cls:
                if n:
                    cls[i, int(rng.integers(0, n))] = k
        passes.append((dict(count=count, conf=conf, cls=cls, box=box), gts))
    return passes


def feed_device(calc, passes, b, out_cap):
    keep = []
    for slots, gts in passes:
        t = {k: torch.from_numpy(v).cuda() for k, v in slots.items()}
        keep.append(t)                                                  # (alive until the stream has run the append)
        calc.add_pass((t['count'].data_ptr(), t['conf'].data_ptr(), t['cls'].data_ptr(), t['box'].data_ptr(), b, out_cap), gts)
    return keep


def feed_host(calc, passes, out_cap, ncls):
    for slots, gts in passes:
        for i, gt in enumerate(gts):
            n = min(int(slots['count'][i]), out_cap)
            ok = [j for j in range(n) if 0 <= slots['cls'][i, j] < ncls]
            det = dict(conf=slots['conf'][i, ok], cls=slots['cls'][i, ok], box=slots['box'][i, ok])
            calc.add_detections(gt, su.boxes_from_detection(det, NAMES))


def oracle_of_passes(passes, out_cap, ncls, protocol, thresholds=(0.5,)):
    """{label: AP} from the oracle on the arrays the host lists would hold"""
    db, dc, dk, ds, gb, gk, gs, gf, first = [], [], [], [], [], [], [], [], []
    sample = 0
    for slots, gts in passes:
        for i, gt in enumerate(gts):
            for g in gt:
                gb.append(prop2abs(g.center, g.size, IMG)); gk.append(g.labelid); gs.append(sample); gf.append(int(getattr(g, 'difficult', False)))
                if g.labelid not in first:
                    first.append(g.labelid)
            for j in range(min(int(slots['count'][i]), out_cap)):
                if 0 <= slots['cls'][i, j] < ncls:
                    db.append(roundtrip(slots['box'][i, j])); dc.append(slots['conf'][i, j]); dk.append(slots['cls'][i, j]); ds.append(sample)
            sample += 1
    ap, present = R.compute(np.array(db, np.float32).reshape(-1, 4), dc, dk, ds, np.array(gb, np.float64).reshape(-1, 4), gk, gs, gf, ncls=ncls,
                            protocol=protocol, minoverlaps=thresholds)
    many = len(thresholds) > 1
    return {NAMES[k]: ([float(v) for v in ap[:, k]] if many else float(ap[0, k])) for k in first if present[k]}, len(dc)


def passes_to_grow_twice(b, out_cap):
    """the buffers start at max(first pass, 1024) detections of room and double: past 2048 of the host's bound they grew twice"""
    per = b * out_cap
    return max(5, 2048 // per + 2) if per < 1024 else 5


def test_roundtrip_is_not_the_identity():
    assert roundtrip(CHANGING) == (989, 1052, 173, 481)


@pytest.mark.parametrize('out_cap', [1, 200])
@pytest.mark.parametrize('b', [1, 33])
def test_accumulator_against_host_lists_and_oracle(b, out_cap):
    ncls = 20
    n_pass = passes_to_grow_twice(b, out_cap)
    passes = make_passes(100 * b + out_cap, b, out_cap, n_pass, ncls)
    assert any(int(s['count'].max()) > out_cap for s, _ in passes) and any(int(s['count'].min()) == 0 for s, _ in passes)
    host = apm.APCalculator()
    feed_host(host, passes, out_cap, ncls)
    want = host.compute_aps()
    calc = apm.DeviceAPCalculator(0, ncls)
    keep = feed_device(calc, passes, b, out_cap)
    got = calc.compute_aps()
    assert list(got.items()) == list(want.items())                     # same keys in the same order, same float64
    assert calc.num_detections() == len(host.det_confidence) and calc.num_dropped() == 0
    assert apm.APs2mAP(got) == apm.APs2mAP(want)
    st = calc.state()
    assert np.array_equal(st['det_box'], np.array(host.det_params, np.float32).reshape(-1, 4))
    assert np.array_equal(st['det_confidence'], np.array(host.det_confidence, np.float32))
    assert np.array_equal(st['det_sample_ids'], np.array(host.det_sample_ids, np.int32))
    if out_cap == 200:
        assert (st['det_box'] == np.array([989, 1052, 173, 481], np.float32)).all(1).any()
    # the other protocols and a threshold list, on the same stored detections
    for protocol in (1, 2):
        calc.protocol = PROTOCOL_NAMES[protocol]
        want_p, n = oracle_of_passes(passes, out_cap, ncls, protocol)
        assert list(calc.compute_aps().items()) == list(want_p.items()) and n == calc.num_detections()
        hostp = apm.APCalculator(protocol=PROTOCOL_NAMES[protocol])
        hostp.merge(host.state())
        assert list(hostp.compute_aps().items()) == list(want_p.items())
    calc.minoverlap = THRESHOLDS[10]
    want_l, _ = oracle_of_passes(passes, out_cap, ncls, 2, THRESHOLDS[10])
    assert calc.compute_aps() == want_l
    # clear, then reuse with other passes
    calc.clear()
    assert calc.num_detections() == 0 and calc.compute_aps() == {}
    calc.protocol, calc.minoverlap = 'reference', 0.5
    again = make_passes(7, b, out_cap, 2, ncls)
    host.clear()
    feed_host(host, again, out_cap, ncls)
    keep += feed_device(calc, again, b, out_cap)
    assert list(calc.compute_aps().items()) == list(host.compute_aps().items())
    calc.close()


def test_two_accumulators_merged_through_state():
    b, out_cap, ncls = 5, 40, 20
    passes = make_passes(3, b, out_cap, 6, ncls)
    one = apm.DeviceAPCalculator(0, ncls, 'voc07')
    keep = feed_device(one, passes, b, out_cap)
    halves = [apm.DeviceAPCalculator(0, ncls, 'voc07') for _ in range(2)]
    keep += feed_device(halves[0], passes[:4], b, out_cap) + feed_device(halves[1], passes[4:], b, out_cap)
    merged = apm.DeviceAPCalculator(0, ncls, 'voc07')
    for h in halves:
        merged.merge(pickle.loads(pickle.dumps(h.state())))
    assert merged.num_detections() == one.num_detections() > 0
    want, _ = oracle_of_passes(passes, out_cap, ncls, 1)
    assert list(merged.compute_aps().items()) == list(one.compute_aps().items()) == list(want.items())
    a, m = one.state(), merged.state()
    for k in ('det_box', 'det_confidence', 'det_classes', 'det_sample_ids'):
        assert np.array_equal(a[k], m[k]), k
    # more passes behind a merge
    keep += feed_device(merged, passes[:1], b, out_cap) + feed_device(one, passes[:1], b, out_cap)
    assert list(merged.compute_aps().items()) == list(one.compute_aps().items())
    for c in [one, merged] + halves:
        c.close()


def test_out_of_range_class_is_counted_not_stored():
    b, out_cap, ncls = 4, 30, 20
    passes = make_passes(9, b, out_cap, 3, ncls, bad_cls=(20, 127, -1))
    bad = sum(int(np.count_nonzero((s['cls'][i, :min(int(s['count'][i]), out_cap)] < 0) | (s['cls'][i, :min(int(s['count'][i]), out_cap)] >= ncls)))
              for s, _ in passes for i in range(b))
    assert bad > 0
    calc = apm.DeviceAPCalculator(0, ncls, 'voc12')
    keep = feed_device(calc, passes, b, out_cap)
    want, n = oracle_of_passes(passes, out_cap, ncls, 2)
    assert list(calc.compute_aps().items()) == list(want.items())
    assert calc.num_detections() == n and calc.num_dropped() == bad
    st = calc.state()
    assert st['det_classes'].min() >= 0 and st['det_classes'].max() < ncls
    calc.close()
    c2 = apm.DeviceAPCalculator(0, 2)
    with pytest.raises(RuntimeError, match='class id'):                 # ground truth outside the class range is refused
        feed_device(c2, [(passes[0][0], [[Box('c5', 5, *abs2prop(1, 5, 1, 5, IMG))]] * b)], b, out_cap)
    assert c2.num_detections() == 0
    c2.close()
    with pytest.raises(RuntimeError):
        apm.DeviceAPCalculator(0, 128)


# ------------------------------------------------------------------------------------- behind real detection passes
def synthetic_gt(rng, n, ncls):
    out = []
    for _ in range(n):
        gt = []
        for _ in range(3):
            x0, y0 = (int(v) for v in rng.integers(0, 600, 2)); w, h = (int(v) for v in rng.integers(100, 400, 2))
            k = int(rng.integers(0, ncls))
            gt.append(Box(NAMES[k], k, *abs2prop(x0, x0 + w, y0, y0 + h, IMG)))
        out.append(gt)
    return out


def test_end_to_end_behind_the_decode():
    from ssd_tensorflow_amd.ssdvgg import SSDVGG, Session
    rng = np.random.default_rng(4)
    ncls = 20
    with Session(0) as sess:
        net = SSDVGG(sess, 'vgg300')
        net.build_from_vgg(None, ncls, max_batch=2, training=False)
        host = apm.APCalculator()
        calc = apm.DeviceAPCalculator(0, ncls)
        pending = None
        total = 0
        for step in range(3):
            x = torch.from_numpy(rng.integers(0, 256, (2, 300, 300, 3)).astype(np.float32)).cuda()
            gts = synthetic_gt(rng, 2, ncls)
            net.infer_dev(x)
            ticket = net.detect_last_launch(2, 0.01, None, 200)
            calc.add_pass(ticket, gts)
            if pending:                                                # collected one pass late, as the drivers do
                for gt, det in zip(pending[1], pending[0].get()):
                    host.add_detections(gt, su.boxes_from_detection(det, NAMES)); total += len(det['conf'])
            pending = (ticket, gts)
        for gt, det in zip(pending[1], pending[0].get()):
            host.add_detections(gt, su.boxes_from_detection(det, NAMES)); total += len(det['conf'])
        assert total == 6 * 200                                         # threshold 0.01 on random weights: the cap fills
        want = host.compute_aps()
        assert list(calc.compute_aps().items()) == list(want.items()) and len(want) > 3
        assert calc.num_detections() == total
        calc.close()


def test_end_to_end_behind_a_tiled_pass(tmp_path):
    from ssd_tensorflow_amd import tiling
    from ssd_tensorflow_amd.ssdvgg import SSDVGG, Session
    rng = np.random.default_rng(6)
    files = []
    for k in range(2):
        files.append(str(tmp_path / ('pic%d.npy' % k)))
        np.save(files[-1], rng.integers(0, 256, (300, 520, 3)).astype(np.uint8))
    ncls = 20
    with Session(0) as sess:
        net = SSDVGG(sess, 'vgg300')
        net.build_from_vgg(None, ncls, max_batch=2, training=False)
        det = tiling.TiledDetector(net, 300, whole=False, threshold=0.01)
        src = next(tiling.source_batches(files, 2, 0))[:3]
        assert [sum(1 for t in det.plan(src[2]) if t[0] == i) for i in range(2)] == [2, 2]
        gts = synthetic_gt(rng, 2, ncls)
        host = apm.APCalculator(protocol='voc12')
        calc = apm.DeviceAPCalculator(0, ncls, 'voc12')
        ticket = det.launch(*src)
        calc.add_pass(ticket, gts)
        n = 0
        for gt, d in zip(gts, ticket.get()):
            host.add_detections(gt, su.boxes_from_detection(d, NAMES)); n += len(d['conf'])
        want = host.compute_aps()
        assert n > 100 and list(calc.compute_aps().items()) == list(want.items()) and calc.num_detections() == n
        calc.close()


# ------------------------------------------------------------------------------------- the drivers
AP_LINE = re.compile(r'^\[i\] (AP \[|mAP|Processed )')


def _infer_child(tmp_path, ap_on, extra=()):
    cmd = [sys.executable, '-m', 'ssd_tensorflow_amd.infer', '--name', str(tmp_path / 'none'), '--preset', 'vgg300', '--synthetic', '8',
           '--synthetic-boxes', '3', '--batch-size', '4', '--threshold', '0.01', '--output-dir', str(tmp_path / ('out_' + ap_on)),
           '--ap-on', ap_on, *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return [l for l in r.stdout.splitlines() if AP_LINE.match(l)], r.stdout


def test_infer_driver_ap_on_gpu_prints_the_host_lines(tmp_path):
    host, _ = _infer_child(tmp_path, 'host')
    gpu, out = _infer_child(tmp_path, 'gpu')
    assert gpu == host and len(host) > 5, (host, gpu)
    assert host[-1] == '[i] Processed 8 images, 1600 detections' and any(l.startswith('[i] mAP') for l in host)
    assert '[i] AP detections on:   gpu' in out


def test_infer_driver_protocols_and_summary_files(tmp_path):
    """voc12 on the GPU with --pascal-summary (the files still need the boxes on the host) against the host lists"""
    host, _ = _infer_child(tmp_path, 'host', ('--ap-protocol', 'voc12', '--pascal-summary', 'true'))
    gpu, _ = _infer_child(tmp_path, 'gpu', ('--ap-protocol', 'voc12', '--pascal-summary', 'true'))
    assert gpu == host and len(host) > 5
    a, b = str(tmp_path / 'out_host'), str(tmp_path / 'out_gpu')
    assert sorted(os.listdir(a)) == sorted(os.listdir(b)) and os.listdir(a)
    for f in os.listdir(a):
        assert open(os.path.join(a, f)).read() == open(os.path.join(b, f)).read(), f


def test_train_driver_ap_on_gpu_prints_the_host_map_lines(tmp_path, capsys):
    from ssd_tensorflow_amd import train
    common = ['--batch-size', '8', '--synthetic-train', '16', '--synthetic-valid', '8', '--synthetic-classes', '1', '--epochs', '2',
              '--checkpoint-interval', '10', '--lr-values', '0.0001', '--lr-boundaries', '', '--tensorboard-dir', str(tmp_path / 'tb')]
    lines = {}
    for ap_on in ('host', 'gpu'):
        assert train.main(['--name', str(tmp_path / ap_on), '--ap-on', ap_on] + common) == 0
        lines[ap_on] = [l for l in capsys.readouterr().out.splitlines() if l.startswith('[i] mAP')]
    assert lines['gpu'] == lines['host'] and len(lines['host']) == 1, lines
