"""-m gpu: Soft-NMS in the DetectionOutput decode through the C ABI and the Python mirrors against the numpy
float32 oracle tests/softnms_ref.py: counts, confidence BITS, classes, anchors (tiles) and boxes compared with np.array_equal, no
tolerance anywhere.  The cases and their oracle results are tests/softnms_cases.py's, computed once per process;
tests/test_softnms_ref.py shows on the CPU what each case is able to see."""
import ctypes as C

import numpy as np
import pytest
import torch

import detout_cases as dc
import softnms_cases as sc
import softnms_ref as sr
import tiledet_ref as tdr
from gpu_util import dev as _dev, host
from ssd_tensorflow_amd import _lib, tiling
from ssd_tensorflow_amd import ssdutils as su
from ssd_tensorflow_amd._lib import lib, last_error, np_ptr, check

pytestmark = pytest.mark.gpu

KINDS = [(sr.LINEAR, 'linear'), (sr.GAUSSIAN, 'gaussian')]
kinds = pytest.mark.parametrize('kind,kname', KINDS, ids=[k[1] for k in KINDS])


def dev(a):
    return _dev(np.array(a))


def params(kind, iou_thr=0.45, sigma=0.5, min_score=0.0):
    return su.NmsParams(kind, iou_thr, sigma, min_score)


def pp(nms):
    return C.cast(C.pointer(nms), C.c_void_p)


# ------------------------------------------------------------------------------------------------ 1. the rule alone
def soft_boxes(conf, box, nms):
    n = len(conf)
    order = np.full(max(n, 1), -1, np.int32)
    out = np.full(max(n, 1), -1, np.float32)
    nk = C.c_int(-1)
    rc = lib.ssd_soft_nms_boxes(0, n, np_ptr(np.ascontiguousarray(box)), np_ptr(np.ascontiguousarray(conf)), pp(nms), np_ptr(order), np_ptr(out),
                                C.byref(nk))
    assert rc == 0, last_error()
    return nk.value, order, out


@kinds
@pytest.mark.parametrize('name', sc.LIST_NAMES)
def test_soft_nms_boxes_equals_the_oracle_twice(name, kind, kname):
    d = sc.list_case(name)
    want_order, want_scores = sc.list_expected(name, kind)
    first = None
    for _ in range(2):
        n, order, out = soft_boxes(d['conf'], d['box'], params(kind, *d['params'][kind]))
        assert n == len(want_order), (n, len(want_order))
        assert np.array_equal(order[:n], want_order), 'pick order'
        assert np.array_equal(out[:n].view(np.uint32), want_scores.view(np.uint32)), 'score bits'
        assert (order[n:] == -1).all() and (out[n:] == -1).all(), 'entries past the count were written'
        assert first is None or (first[0] == n and np.array_equal(first[1], order) and np.array_equal(first[2].view(np.uint32), out.view(np.uint32)))
        first = (n, order, out)


def test_soft_nms_boxes_python_mirror_and_refusals():
    d = sc.list_case('overlap-65')
    order, scores = su.soft_nms_boxes(d['conf'], d['box'], 'gaussian', 0.45, 0.5, 0.01)
    want = sc.list_expected('overlap-65', sr.GAUSSIAN)
    assert np.array_equal(order, want[0]) and np.array_equal(scores.view(np.uint32), want[1].view(np.uint32))
    assert su.soft_nms_boxes(np.zeros(0, np.float32), np.zeros((0, 4), np.int32))[0].size == 0
    nk = C.c_int(0)
    z = np.zeros(4 * 1025, np.int32)
    for n, box, conf, what in ((1025, z, z.view(np.float32), '0..1024'),
                               (1, np.array([5, 4, 0, 9], np.int32), np.ones(1, np.float32), '1000 grid'),
                               (1, np.array([0, 1000, 0, 9], np.int32), np.ones(1, np.float32), '1000 grid'),
                               (1, np.array([0, 9, 0, 9], np.int32), np.array([-0.0], np.float32), 'non-negative'),
                               (1, np.array([0, 9, 0, 9], np.int32), np.array([np.nan], np.float32), 'non-negative')):
        assert lib.ssd_soft_nms_boxes(0, n, np_ptr(box), np_ptr(conf), pp(params(sr.LINEAR)), np_ptr(z), np_ptr(z.view(np.float32)), C.byref(nk)) != 0
        assert what in last_error(), last_error()
        assert not z.any()


# ------------------------------------------------------------------------------------------------ 2. images
def host_entry(pname, pred, thr, k, keep, out_cap, nms):
    b, A, nv = pred.shape
    count = np.full(b, -1, np.int32)
    conf = np.full((b, out_cap), -1, np.float32)
    cls, idx = np.full((b, out_cap), -1, np.int32), np.full((b, out_cap), -1, np.int32)
    box = np.full((b, out_cap, 4), -1, np.int32)
    rc = lib.ssd_detection_output_soft(pname.encode(), nv - 5, 0, np_ptr(pred), b, thr, k, keep, out_cap, np_ptr(count), np_ptr(conf), np_ptr(cls),
                                       np_ptr(idx), np_ptr(box), pp(nms))
    assert rc == 0, last_error()
    return count, conf, cls, idx, box


_ANCHORS_DEV = {}


def anchors_dev(pname):
    if pname not in _ANCHORS_DEV:
        _ANCHORS_DEV[pname] = dev(su.anchors_array(pname))
    return _ANCHORS_DEV[pname]


def dev_entry(pname, pred, thr, k, keep, out_cap, nms, ws_short=0, pred_dev=None, soft=True):
    """-> (rc, outputs); the outputs start as -1 everywhere, so a row the pass did not write shows"""
    b, A, nv = pred.shape
    need = lib.ssd_detection_output_ws_bytes(pname.encode(), nv - 5, b, k)
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device='cuda:0')
    d_pred = dev(pred) if pred_dev is None else pred_dev
    count = torch.full((b,), -1, dtype=torch.int32, device='cuda:0')
    conf = torch.full((b, out_cap), -1, dtype=torch.float32, device='cuda:0')
    cls, idx = (torch.full((b, out_cap), -1, dtype=torch.int32, device='cuda:0') for _ in range(2))
    box = torch.full((b, out_cap, 4), -1, dtype=torch.int32, device='cuda:0')
    torch.cuda.synchronize()
    args = (pname.encode(), nv - 5, anchors_dev(pname).data_ptr(), d_pred.data_ptr(), b, thr, k, keep, out_cap, count.data_ptr(), conf.data_ptr(),
            cls.data_ptr(), idx.data_ptr(), box.data_ptr(), ws.data_ptr(), need - ws_short)
    stream = torch.cuda.current_stream().cuda_stream
    rc = lib.ssd_detection_output_soft_dev(*args, pp(nms), stream) if soft else lib.ssd_detection_output_dev(*args, stream)
    return rc, tuple(host(t) for t in (count, conf, cls, idx, box))


def check_against(want, outs, out_cap, untouched=None):
    count, conf, cls, idx, box = outs
    for i, w in enumerate(want):
        n = len(w['idx'])
        assert count[i] == n, f'image {i}: count {count[i]} != {n}'
        m = min(n, out_cap)
        assert np.array_equal(conf[i, :m].view(np.uint32), w['conf'][:m].view(np.uint32)), f'image {i}: confidence bits'
        assert np.array_equal(cls[i, :m], w['cls'][:m]), f'image {i}: classes'
        assert np.array_equal(idx[i, :m], w['idx'][:m]), f'image {i}: anchors'
        assert np.array_equal(box[i, :m], w['box'][:m]), f'image {i}: boxes'
        if untouched is not None:       # rows past the count: zero from the host entry, not written by the device entry
            assert (conf[i, m:] == untouched).all() and (cls[i, m:] == untouched).all() and (idx[i, m:] == untouched).all()
            assert (box[i, m:] == untouched).all()


def image_params(name, kind):
    pname, pred, thr, k, keep, min_score = sc.image_case(name)
    return params(kind, 0.45, 0.5, thr if min_score is None else min_score)


@kinds
@pytest.mark.parametrize('name', sc.IMAGE_NAMES)
def test_host_entry_equals_the_oracle(name, kind, kname):
    pname, pred, thr, k, keep, _ = sc.image_case(name)
    before = pred.copy()
    outs = host_entry(pname, pred, thr, k, keep, keep, image_params(name, kind))
    assert np.array_equal(pred, before), 'pred must not be modified'
    check_against(sc.image_expected(name, kind), outs, keep, untouched=0)


@kinds
@pytest.mark.parametrize('name', sc.IMAGE_NAMES)
def test_dev_entry_equals_the_oracle(name, kind, kname):
    pname, pred, thr, k, keep, _ = sc.image_case(name)
    d_pred = dev(pred)
    rc, outs = dev_entry(pname, pred, thr, k, keep, keep, image_params(name, kind), pred_dev=d_pred)
    assert rc == 0, last_error()
    assert np.array_equal(host(d_pred), pred), 'pred must not be modified'
    check_against(sc.image_expected(name, kind), outs, keep, untouched=-1)


@pytest.mark.parametrize('name', ['softmax-C3', 'softmax-vgg512-C3', 'sparse', 'cut-ties'])
def test_kind_hard_through_the_new_entries_is_byte_equal(name):
    pname, pred, thr, k, keep = dc.case(name)
    garbage = su.NmsParams(0, float('nan'), -1.0, float('-inf'))      # kind = hard reads no other field
    rc, want = dev_entry(pname, pred, thr, k, keep, keep, None, soft=False)
    assert rc == 0, last_error()
    rc, got = dev_entry(pname, pred, thr, k, keep, keep, garbage)
    assert rc == 0, last_error()
    assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want))
    got = host_entry(pname, pred, thr, k, keep, keep, garbage)
    b = pred.shape[0]
    ref = [np.full(b, -1, np.int32), np.full((b, keep), -1, np.float32)] + [np.full((b, keep), -1, np.int32) for _ in range(2)]
    ref.append(np.full((b, keep, 4), -1, np.int32))
    assert lib.ssd_detection_output(pname.encode(), pred.shape[2] - 5, 0, np_ptr(pred), b, thr, k, keep, keep, *[np_ptr(a) for a in ref]) == 0
    assert all(g.tobytes() == w.tobytes() for g, w in zip(got, ref))
    assert got[0].max() > 50


@kinds
@pytest.mark.parametrize('entry', ['host', 'dev'])
def test_out_cap_below_the_count_clips_rows(entry, kind, kname):
    pname, pred, thr, k, keep, _ = sc.image_case('softmax-C3')
    want = sc.image_expected('softmax-C3', kind)
    assert min(len(w['idx']) for w in want) > 50
    nms = image_params('softmax-C3', kind)
    if entry == 'host':
        outs = host_entry(pname, pred, thr, k, keep, 50, nms)
    else:
        rc, outs = dev_entry(pname, pred, thr, k, keep, 50, nms)
        assert rc == 0, last_error()
    assert outs[1].shape == (3, 50)
    check_against(want, outs, 50)


def test_a_short_workspace_and_bad_parameters_launch_nothing():
    pname, pred, thr, k, keep, _ = sc.image_case('nms-top-k-1')
    for nms, short, what in ((params(sr.LINEAR), 1, 'workspace'), (su.NmsParams(3, 0.45, 0.5, 0.0), 0, 'nms kind'),
                             (params(sr.LINEAR, iou_thr=1.5), 0, 'iou_thr'), (params(sr.GAUSSIAN, sigma=0.0), 0, 'sigma'),
                             (params(sr.GAUSSIAN, min_score=-1.0), 0, 'min_score')):
        rc, outs = dev_entry(pname, pred, thr, k, keep, keep, nms, ws_short=short)
        assert rc != 0 and what in last_error(), (what, last_error())
        assert all((o == -1).all() for o in outs), what + ': an output was written'


def test_python_mirror_takes_the_keywords():
    pname, pred, thr, k, keep, _ = sc.image_case('full-frame')
    preset = su.get_preset_by_name(pname)
    for kind, kname in KINDS:
        got = su.detection_output_batch(pred, preset, thr, k, keep, soft_nms=kname)
        for g, w in zip(got, sc.image_expected('full-frame', kind)):
            assert sr_same(g, w)
        boxes = su.detection_output(pred[0], pname, thr, {}, k, keep, soft_nms=kname)
        assert [float(c) for c, _ in boxes] == [float(c) for c in sc.image_expected('full-frame', kind)[0]['conf']]
    got = su.detection_output_batch(pred, preset, thr, k, keep, soft_nms='gaussian', soft_nms_sigma=0.3, soft_nms_min_score=0.05)
    want = [sr.detection_output(pred[i], dc.anchors(pname), thr, k, keep, sr.GAUSSIAN, 0.45, 0.3, 0.05) for i in range(2)]
    assert all(sr_same(g, w) for g, w in zip(got, want)) and all((w['conf'] >= np.float32(0.05)).all() for w in want)
    with pytest.raises(ValueError, match='soft_nms'):
        su.detection_output_batch(pred, preset, thr, k, keep, soft_nms='matrix')
    with pytest.raises(RuntimeError, match='sigma'):
        su.detection_output_batch(pred, preset, thr, k, keep, soft_nms='gaussian', soft_nms_sigma=-1.0)


def sr_same(got, want, tile=False):
    keys = ('cls', 'idx', 'box') + (('tile',) if tile else ())
    return (len(got['idx']) == len(want['idx']) and np.array_equal(got['conf'].view(np.uint32), want['conf'].view(np.uint32))
            and all(np.array_equal(got[k], want[k]) for k in keys))


# ------------------------------------------------------------------------------------------------ 3. tiled
def _tl(tiles):
    return [(i, tiling.Tile(*t), s) for i, t, s in tiles]


@kinds
def test_tiled_host_and_device_entries_equal_the_tiled_oracle(kind, kname):
    pname, thr, k, keep, m = sc.TILED
    pred, tiles = sc.tiled_case()
    want = sc.tiled_expected(kind)
    assert all(len(w['idx']) == keep for w in want) and any(len(set(w['tile'].tolist())) > 2 for w in want)
    hard = tdr.detout_tiles_all(pred, tiles, dc.anchors(pname), thr, k, keep, m)
    assert not all(tdr.same(h, w) for h, w in zip(hard, want)), 'the case does not tell the soft rule from the hard one'
    got = su.detect_tiles(pred, su.get_preset_by_name(pname), _tl(tiles), thr, edge_margin=m, decode='all', nms_top_k=k, keep_top_k=keep,
                          soft_nms=kname)
    assert len(got) == 2 and all(sr_same(g, w, tile=True) for g, w in zip(got, want))
    # the device entries: the tile stage as it is, in two calls, then the soft merge
    tl = _tl(tiles)
    n_tiles, A, nv = pred.shape
    d = torch.device('cuda', _lib.device())
    wsb = int(lib.ssd_detout_tiles_ws_bytes(pname.encode(), nv - 5, n_tiles, 2, k))
    ws = torch.empty(wsb, dtype=torch.uint8, device=d)
    structs = C.cast(tiling.tile_structs(tl), C.c_void_p)
    o = {key: torch.full((2, keep, 4) if key == 'box' else (2, keep), -7, dtype=torch.float32 if key == 'conf' else torch.int32, device=d)
         for key in ('conf', 'cls', 'idx', 'tile', 'box')}
    count = torch.full((2,), -7, dtype=torch.int32, device=d)
    for first, b in ((0, 3), (3, 5)):
        x = torch.tensor(pred[first:first + b], device=d)
        check(lib.ssd_detout_tiles_add_dev(pname.encode(), nv - 5, anchors_dev(pname).data_ptr(), x.data_ptr(), structs, n_tiles, first, b, thr, k, m,
                                           ws.data_ptr(), wsb, None))
    nms = params(kind, 0.45, 0.5, thr)
    assert lib.ssd_detout_tiles_merge_soft_dev(nv - 5, structs, n_tiles, 2, k, keep, keep, count.data_ptr(), o['conf'].data_ptr(), o['cls'].data_ptr(),
                                               o['idx'].data_ptr(), o['tile'].data_ptr(), o['box'].data_ptr(), ws.data_ptr(), wsb - 1, pp(nms),
                                               None) != 0 and 'workspace' in last_error()
    check(lib.ssd_detout_tiles_merge_soft_dev(nv - 5, structs, n_tiles, 2, k, keep, keep, count.data_ptr(), o['conf'].data_ptr(), o['cls'].data_ptr(),
                                              o['idx'].data_ptr(), o['tile'].data_ptr(), o['box'].data_ptr(), ws.data_ptr(), wsb, pp(nms), None))
    raw = {key: host(v) for key, v in o.items()}
    assert host(count).tolist() == [keep, keep]
    for i, w in enumerate(want):
        assert sr_same({key: raw[key][i] for key in raw}, w, tile=True), i


@kinds
def test_a_one_window_picture_equals_the_untiled_entry_byte_for_byte(kind, kname):
    pname, pred, thr, k, keep, _ = sc.image_case('full-frame')
    nms = params(kind, 0.45, 0.5, thr)
    want = host_entry(pname, pred[:1], thr, k, keep, keep, nms)
    tl = [(0, tiling.Tile(0, 0, 640, 480, 0), (640, 480))]
    count = np.full(1, -1, np.int32)
    conf = np.full((1, keep), -1, np.float32)
    cls, idx, tile = (np.full((1, keep), -1, np.int32) for _ in range(3))
    box = np.full((1, keep, 4), -1, np.int32)
    check(lib.ssd_detout_tiles_soft(pname.encode(), pred.shape[2] - 5, 0, np_ptr(pred[:1]), C.cast(tiling.tile_structs(tl), C.c_void_p), 1, 1, thr, k,
                                    keep, 2, keep, np_ptr(count), np_ptr(conf), np_ptr(cls), np_ptr(idx), np_ptr(tile), np_ptr(box), pp(nms)))
    assert count[0] == want[0][0] > 20 and not tile.any()
    for g, w in zip((conf, cls, idx, box), want[1:]):
        assert g.tobytes() == w.tobytes()


# ------------------------------------------------------------------------------------------------ 4. through a handle
def test_handle_detect_last_soft_and_the_default_pass_profile():
    from ssd_tensorflow_amd.ssdvgg import SSDVGG, Session
    ncls, b = 3, 2
    rng = np.random.default_rng(8)
    anch = dc.anchors('vgg300')
    with Session(0) as sess:
        net = SSDVGG(sess, 'vgg300')
        net.build_from_vgg(None, ncls, max_batch=b, training=False, seed=7)
        x = torch.from_numpy(rng.integers(0, 256, (b, 300, 300, 3)).astype(np.float32)).cuda()
        net.infer_dev(x)
        pred = net._dev_result(b, True)
        for kind, kname in KINDS:
            dets = net.detect_last(b, 0.01, decode='all', soft_nms=kname)
            tuned = net.detect_last(b, 0.01, decode='all', nms_top_k=50, keep_top_k=30, soft_nms=kname, soft_nms_iou=0.3, soft_nms_sigma=0.25,
                                    soft_nms_min_score=0.02)
            for i in range(b):
                want = sr.detection_output(pred[i], anch, 0.01, 400, 200, kind)
                assert len(want['idx']) > 20
                assert sr_same(dets[i], want), (kname, i)
                assert sr_same(tuned[i], sr.detection_output(pred[i], anch, 0.01, 50, 30, kind, 0.3, 0.25, 0.02)), (kname, i, 'tuned')
        hard = net.detect_last(b, 0.01, decode='all')
        assert any(not sr_same(hard[i], dets[i]) for i in range(b))
        with pytest.raises(ValueError, match="decode='all'"):
            net.detect_last_launch(b, 0.01, soft_nms='linear')
        with pytest.raises(ValueError, match='soft_nms'):
            net.detect_last_launch(b, 0.01, decode='all', soft_nms='hard')
        with pytest.raises(RuntimeError, match='iou_thr'):
            net.detect_last_launch(b, 0.01, decode='all', soft_nms='linear', soft_nms_iou=2.0)
        # the labels a default pass puts into the profile report are the ones it put there before there was a choice

        def labels(**kw):
            check(lib.ssd_profile_enable(net._h, 1))
            net.detect_last(b, 0.01, decode='all', **kw)
            torch.cuda.synchronize()
            buf = C.create_string_buffer(1 << 16)
            check(lib.ssd_profile_report(net._h, buf, len(buf)))
            check(lib.ssd_profile_enable(net._h, 0))
            return [ln.split('\t')[0] for ln in buf.value.decode().strip().split('\n') if ln]

        default, soft = labels(), labels(soft_nms='gaussian')
        assert sorted(k for k in default if 'det' in k) == ['detout_class', 'detout_merge'], default
        assert sorted(k for k in soft if 'det' in k) == ['detout_class_soft', 'detout_merge'], soft
