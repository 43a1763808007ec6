"""-m gpu: the argmax decode + per-class NMS and ssd_nms_boxes on the crafted cases of tests/decode_cases.py (what each case
hits is proven on the CPU by tests/test_decode_cases.py).

Every image runs through ssd_decode_nms (host pointers) and ssd_decode_nms_dev (resident), the latter twice: with its
workspace pre-filled with 0xFF and with 0x00, its outputs pre-filled with a pattern, guard words in front of and behind every
buffer.  count / idx / cls / box are compared with np.array_equal and conf by its bits against decode_cases.expected()
(ob.decode + ob.suppress): no tolerance anywhere.  The images of one (preset, class count) are stacked by call parameters
(decode_cases.batches), so most of them share two launches; an image's expected result is its own (b = 1) oracle result, so
a batch also shows that neighbours do not leak into each other.

Not reachable: the scalar tail loop of the scan kernels (`for i = (n4 << 2) + t ...`) -- both presets' anchor counts are
multiples of 4, so a block's floats always are.

Wall time on an MI355X: 37 tests in 16.3 s, the slowest 3.4 s (vgg512, 20 classes: the oracle on three images in which every
anchor is a candidate); the oracle results are computed once per process and shared.

What the tests catch -- one-line, memory-safe edits of comparisons in csrc/boxes.hip, one library build each, run once against
this file and against the decode / NMS tests from before it (test_gpu_boxes.py, test_gpu_detection_output.py); the same table is
profiles/decode_edges_mutations.txt:

edit (where)                                                    new tests that fail                                              earlier tests that fail
--------------------------------------------------------------  ---------------------------------------------------------------  -----------------------
!(conf < thr) -> conf > thr (detect_scan_block)                 batches vgg300-C20 parts 0-3                                     none
!(conf < thr) -> conf > thr (detect_scan_wide_kernel)           batches vgg300-C28 (no test failed before the threshold cases
                                                                were added at C = 28)                                            none
r[c] > conf -> >= (detect_scan_block)                           batches vgg300-C20 parts 0-2, vgg300-C27, vgg512-C20             none
ob < best -> ob > best (detect_scan_wide_kernel)                batches vgg300-C28, vgg300-C127, vgg512-C28                      none
20 * inter > 9 * uni -> >= (overlaps45)                         batches vgg300-C20 parts 0-1, vgg512-C20, vgg512-C28             none
the hi loop of nms_segment skipped (for i = len; ...)           batches vgg300-C20 parts 0, 2, 3, vgg300-C1, -C27, -C28, -C127,  test_detect_fast_and_general_paths_agree_with_oracle,
                                                                vgg512-C20; test_one_image_five_times                            test_{host,dev}_entry_equals_the_oracle[one-class]
loc[e] > 100.f -> > 99.f (decode_box)                           batches vgg300-C20 parts 0-1                                     none
conf[i] == 0.f ? 0.f : conf[i] -> conf[i] (nms_boxes_kernel:    test_nms_boxes_cases[zeros-neg-first, zeros-mixed, zeros-groups,
the order before this change, -0.0 below +0.0)                  zeros-overlap]; test_suppress_overlaps_ties_negatives_and_label_ids  none

Not run: (32767 - a) -> a in the scan key.  detect_image_kernel takes the anchor back out of the key to address pred and the
anchor table, so the edit moves an index: with A = 8732 every read would land 24 035 .. 32 767 rows in, beyond both arrays.
The order it would produce (equal confidences by HIGHER anchor) is the 'tie-high-anchor' switch of tests/test_decode_cases.py,
under which the expected result of every ties case changes.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import decode_cases as dc
from oracle import boxes as ob
from gpu_util import DEV
from ssd_tensorflow_amd import _lib, ssdutils as su
from ssd_tensorflow_amd._lib import lib, check, np_ptr
from ssd_tensorflow_amd.utils import Box, Point, Size

pytestmark = pytest.mark.gpu
GUARD = 64                                  # int32 words in front of and behind every buffer
GUARDW = 0x7B7B7B7B
PAT = 0x5A5A5A5A                            # what the outputs hold before the call


class _Buf:
    """[guard | words | guard] int32 on the device; .ptr addresses the payload"""
    def __init__(self, words, fill):
        self.words = int(words)
        self.t = torch.full((self.words + 2 * GUARD,), fill, dtype=torch.int32, device=DEV)
        self.t[:GUARD] = GUARDW
        self.t[GUARD + self.words:] = GUARDW
        self.ptr = self.t.data_ptr() + 4 * GUARD

    def read(self):
        """-> payload as int32 numpy; asserts the guards"""
        h = self.t.cpu().numpy()
        assert (h[:GUARD] == GUARDW).all() and (h[GUARD + self.words:] == GUARDW).all(), 'a guard word was written'
        return h[GUARD:GUARD + self.words].copy()


@pytest.fixture(scope='module')
def anchors_dev():
    out = {}
    for pname, A in dc.A_OF.items():
        t = torch.empty((A, 4), dtype=torch.float64, device=DEV)
        check(lib.ssd_anchors_dev(pname.encode(), t.data_ptr(), None, None))
        out[pname] = t
    torch.cuda.synchronize()
    return out


def _args(params):
    pname, ncls, thr, cap, max_out, out_cap, nms = params
    return pname.encode(), ncls, thr, -1 if cap is None else cap, -1 if max_out is None else max_out, out_cap, nms


def _run_dev(params, pred, anchors, ws_fill):
    """ssd_decode_nms_dev -> (count [b], conf bits [b, out_cap], cls, idx, box [b, out_cap, 4]); outputs pre-filled with PAT"""
    pname, ncls, thr, cap, mo, out_cap, nms = _args(params)
    b = pred.shape[0]
    dpred = _Buf(pred.size, 0)
    dpred.t[GUARD:GUARD + pred.size] = torch.from_numpy(pred.reshape(-1).view(np.int32)).to(DEV)
    ws = _Buf((int(lib.ssd_decode_nms_ws_bytes(pname, b)) + 3) // 4, -1 if ws_fill == 0xFF else 0)
    count, conf, cls, idx = _Buf(b, PAT), _Buf(b * out_cap, PAT), _Buf(b * out_cap, PAT), _Buf(b * out_cap, PAT)
    box = _Buf(b * out_cap * 4, PAT)
    check(lib.ssd_decode_nms_dev(pname, ncls, anchors.data_ptr(), dpred.ptr, b, thr, cap, mo, out_cap, nms, count.ptr, conf.ptr,
                                 cls.ptr, idx.ptr, box.ptr, ws.ptr, None))
    torch.cuda.synchronize()
    ws.read()
    assert np.array_equal(dpred.read(), pred.reshape(-1).view(np.int32)), 'pred must not be modified'
    return (count.read(), conf.read().view(np.uint32).reshape(b, out_cap), cls.read().reshape(b, out_cap),
            idx.read().reshape(b, out_cap), box.read().reshape(b, out_cap, 4))


def _run_host(params, pred):
    """ssd_decode_nms -> the same tuple (rows past an image's count are unspecified here: the call copies its own device
    buffers back whole)"""
    pname, ncls, thr, cap, mo, out_cap, nms = _args(params)
    b = pred.shape[0]

    def arr(words):
        a = np.full(words + 2 * GUARD, PAT, np.int32)
        a[:GUARD] = GUARDW; a[GUARD + words:] = GUARDW
        return a
    bufs = [arr(b), arr(b * out_cap), arr(b * out_cap), arr(b * out_cap), arr(b * out_cap * 4)]
    before = pred.copy()
    check(lib.ssd_decode_nms(pname, ncls, _lib.device(), np_ptr(pred), b, thr, cap, mo, out_cap, nms,
                             *[C.c_void_p(a.ctypes.data + 4 * GUARD) for a in bufs]))
    assert np.array_equal(pred.view(np.int32), before.view(np.int32)), 'pred must not be modified'
    for a in bufs:
        assert (a[:GUARD] == GUARDW).all() and (a[-GUARD:] == GUARDW).all(), 'a guard word was written'
    count, conf, cls, idx, box = [a[GUARD:-GUARD] for a in bufs]
    return count, conf.view(np.uint32).reshape(b, out_cap), cls.reshape(b, out_cap), idx.reshape(b, out_cap), box.reshape(b, out_cap, 4)


def _compare(got, group, out_cap, untouched_rest, what):
    count, conf, cls, idx, box = got
    for i, case in enumerate(group):
        want = dc.expected(case)
        tag = '%s image %d (%s)' % (what, i, case.name)
        assert count[i] == want['count'], tag
        k = min(want['count'], out_cap)
        assert np.array_equal(idx[i, :k], want['idx'][:k]), tag
        assert np.array_equal(cls[i, :k], want['cls'][:k]), tag
        assert np.array_equal(conf[i, :k], want['conf'][:k].view(np.uint32)), tag
        assert np.array_equal(box[i, :k], want['box'][:k]), tag
        if untouched_rest:      # rows past the count and past out_cap keep what the caller put there
            p = np.uint32(PAT)
            assert (conf[i, k:] == p).all() and (cls[i, k:] == PAT).all() and (idx[i, k:] == PAT).all() and (box[i, k:] == PAT).all(), tag


def _run_groups(groups, anchors_dev):
    for params, group in groups:
        pred = dc.stack(group)
        out_cap = params[5]
        _compare(_run_host(params, pred), group, out_cap, False, 'host')
        for fill in (0xFF, 0x00):
            _compare(_run_dev(params, pred, anchors_dev[params[0]], fill), group, out_cap, True, 'dev ws=%02x' % fill)


PARTS = [(pname, ncls, part) for pname, ncls in dc.COMBOS for part in range(4 if (pname, ncls) == ('vgg300', 20) else 1)]


@pytest.mark.parametrize('pname,ncls,part', PARTS, ids=['%s-C%d-%d' % p for p in PARTS])
def test_decode_cases_in_batches(pname, ncls, part, anchors_dev):
    """every crafted image of the (preset, class count), stacked by call parameters, through both entry points"""
    groups = dc.batches(pname, ncls)
    nparts = 4 if (pname, ncls) == ('vgg300', 20) else 1
    _run_groups(groups[part::nparts], anchors_dev)


def test_one_image_five_times(anchors_dev):
    """b = 5 of the same image: five identical, correct results (every scan block that straddles two images sees equal ones)"""
    for name in ('segment-65-broken', 'ties-800', 'count-2049-nms'):
        case = next(c for c in dc.cases('vgg300', 20) if c.name == name)
        group = [case] * 5
        for got, rest, what in ((_run_host(case.params, dc.stack(group)), False, 'host'),
                                (_run_dev(case.params, dc.stack(group), anchors_dev['vgg300'], 0xFF), True, 'dev')):
            _compare(got, group, case.out_cap, rest, what)
            n = min(int(got[0][0]), case.out_cap)
            for a in got[1:]:
                assert all(np.array_equal(a[0, :n], a[i, :n]) for i in range(1, 5)), name


def test_cap_zero_writes_nothing(anchors_dev):
    """cap = 0 through the C ABI (the Python wrappers map None to -1 and never pass 0): no candidate is kept"""
    case = next(c for c in dc.cases('vgg300', 20) if c.name == 'cap-600-0')
    assert case.cap == 0 and dc.expected(case)['count'] == 0
    got = _run_dev(case.params, dc.stack([case]), anchors_dev['vgg300'], 0xFF)
    assert got[0][0] == 0
    _compare(got, [case], case.out_cap, True, 'dev')


# ---- ssd_nms_boxes ------------------------------------------------------------------------------------------------------
def _nms_boxes(boxes, conf, group, thr):
    n = len(conf)
    keep = np.full(n + 2, PAT, np.int32)
    nk = C.c_int(-7)
    rc = lib.ssd_nms_boxes(_lib.device(), n, np_ptr(boxes), np_ptr(conf), np_ptr(group), thr, C.c_void_p(keep.ctypes.data + 4), C.byref(nk))
    return rc, keep, nk.value


@pytest.mark.parametrize('name', [c[0] for c in dc.nms_cases()])
def test_nms_boxes_cases(name):
    _, boxes, conf, group, thr, edge = next(c for c in dc.nms_cases() if c[0] == name)
    want = dc.nms_expected(boxes, conf, group, thr)
    rc, keep, nk = _nms_boxes(boxes, conf, group, thr)
    assert rc == 0, _lib.last_error()
    assert nk == len(want) and list(keep[1:1 + nk]) == want
    assert keep[0] == PAT and (keep[1 + nk:] == PAT).all()


def test_nms_boxes_65536_refused():
    n = 65536
    boxes = np.zeros((n, 4), np.int32); conf = np.zeros(n, np.float32)
    rc, keep, nk = _nms_boxes(boxes, conf, None, 0.45)
    assert rc != 0 and _lib.last_error() == 'ssd_nms_boxes: 0..65535 boxes (got 65536)'
    assert (keep == PAT).all() and nk == -7
    with pytest.raises(ValueError, match='at most 65535 boxes'):
        su.non_maximum_suppression([(0.5, Box('a', 0, Point(0.5, 0.5), Size(0.1, 0.1)))] * n, 0.45)


def test_suppress_overlaps_ties_negatives_and_label_ids():
    """heavy ties (both zeros among them), negative confidences and arbitrary label ids through the Python entry points: class
    groups in first-appearance order, equal confidences by position in the list"""
    rng = np.random.default_rng(58)
    n = 300
    cx = rng.uniform(0.1, 0.9, n); cy = rng.uniform(0.1, 0.9, n)
    w = rng.uniform(0.05, 0.4, n); h = rng.uniform(0.05, 0.4, n)
    conf = (np.round(rng.uniform(-0.5, 0.5, n) * 4) / 4).astype(np.float32)            # -0.5 ... 0.5 in quarters, -0.0 and +0.0
    assert np.signbit(conf[conf == 0]).any() and not np.signbit(conf[conf == 0]).all()
    lab = rng.integers(0, 6, n) * 7 - 3
    boxes = [(conf[i], Box('c%d' % lab[i], int(lab[i]), Point(float(cx[i]), float(cy[i])), Size(float(w[i]), float(h[i])))) for i in range(n)]
    recs = [(float(c), b.labelid, ob.prop2abs(b.center.x, b.center.y, b.size.w, b.size.h)) for c, b in boxes]
    got = su.suppress_overlaps(boxes)
    assert [next(i for i, bx in enumerate(boxes) if bx is g) for g in got] == ob.suppress_list(recs, 0.45)
    one = [bx for bx in boxes if bx[1].labelid == boxes[0][1].labelid]
    for thr in (0.0, 0.3, 1.0):
        got = su.non_maximum_suppression(one, thr)
        want = ob.nms_list([(float(c), ob.prop2abs(b.center.x, b.center.y, b.size.w, b.size.h)) for c, b in one], thr)
        assert [next(i for i, bx in enumerate(one) if bx is g) for g in got] == want, thr
