"""GPU: tiled detection with the DetectionOutput decode -- ssd_detout_tiles, ssd_detout_tiles_add_dev /
ssd_detout_tiles_merge_dev and tiling.TiledDetector(decode='all') -- against the numpy oracle tests/tiledet_ref.py, for exact equality
of count, confidence bits, class, anchor, tile and box.  The cases and their oracle results are tests/tiledet_cases.py's;
tests/test_tiledet_ref.py shows on the CPU that they tell every mutant of the oracle from it."""
import ctypes as C

import numpy as np
import pytest
import torch

import detout_cases as DC
import tiledet_cases as TC
from ssd_tensorflow_amd import _lib, tiling
from ssd_tensorflow_amd import ssdutils as su
from ssd_tensorflow_amd._lib import lib, np_ptr, check

pytestmark = pytest.mark.gpu

KEYS = ('conf', 'cls', 'idx', 'tile', 'box')


def _same(got, want, what):
    assert len(got['idx']) == len(want['idx']), (what, len(got['idx']), len(want['idx']))
    assert np.array_equal(got['conf'].view(np.uint32), np.asarray(want['conf'], np.float32).view(np.uint32)), (what, 'conf')
    for k in ('cls', 'idx', 'tile', 'box'):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k)


def _tl(tiles):
    return [(i, tiling.Tile(*t), s) for i, t, s in tiles]


def _host(name, **kw):
    pname, pred, tiles, thr, k, keep, m = TC.case(name)
    a = dict(thr=thr, nms_top_k=k, keep_top_k=keep, edge_margin=m)
    a.update(kw)
    return su.detect_tiles(pred, su.get_preset_by_name(pname), _tl(tiles), a['thr'], edge_margin=a['edge_margin'], decode='all',
                           nms_top_k=a['nms_top_k'], keep_top_k=a['keep_top_k'])


def _dev(name, splits, out_cap=None, fill=-7):
    """the device entry points on torch tensors: one ssd_detout_tiles_add_dev per chunk of `splits`, one merge; the raw output
    arrays, prefilled with `fill`"""
    pname, pred, tiles, thr, k, keep, m = TC.case(name)
    tl = _tl(tiles)
    n_tiles, A, nv = pred.shape
    n_images = tl[-1][0] + 1
    out_cap = keep if out_cap is None else out_cap
    dev = torch.device('cuda', _lib.device())
    anc = torch.empty((A, 4), dtype=torch.float64, device=dev)
    check(lib.ssd_anchors_dev(pname.encode(), anc.data_ptr(), None, None))
    wsb = int(lib.ssd_detout_tiles_ws_bytes(pname.encode(), nv - 5, n_tiles, n_images, k))
    assert wsb > 0
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    structs = C.cast(tiling.tile_structs(tl), C.c_void_p)
    o = dict(count=torch.full((n_images,), fill, dtype=torch.int32, device=dev),
             conf=torch.full((n_images, out_cap), fill, dtype=torch.float32, device=dev),
             cls=torch.full((n_images, out_cap), fill, dtype=torch.int32, device=dev),
             idx=torch.full((n_images, out_cap), fill, dtype=torch.int32, device=dev),
             tile=torch.full((n_images, out_cap), fill, dtype=torch.int32, device=dev),
             box=torch.full((n_images, out_cap, 4), fill, dtype=torch.int32, device=dev))
    first = 0
    for b in splits:
        x = torch.tensor(pred[first:first + b], device=dev)
        check(lib.ssd_detout_tiles_add_dev(pname.encode(), nv - 5, anc.data_ptr(), x.data_ptr(), structs, n_tiles, first, b, thr, k, m,
                                           ws.data_ptr(), wsb, None))
        first += b
    assert first == n_tiles
    check(lib.ssd_detout_tiles_merge_dev(nv - 5, structs, n_tiles, n_images, k, keep, out_cap, o['count'].data_ptr(), o['conf'].data_ptr(),
                                         o['cls'].data_ptr(), o['idx'].data_ptr(), o['tile'].data_ptr(), o['box'].data_ptr(), ws.data_ptr(), wsb,
                                         None))
    torch.cuda.synchronize()
    return {k_: v.cpu().numpy() for k_, v in o.items()}


def _rows(raw, i, out_cap):
    n = min(int(raw['count'][i]), out_cap)
    return {k: raw[k][i, :n] for k in KEYS}


# ------------------------------------------------------------------------------------------------ 1. every case against the oracle
@pytest.mark.parametrize('name', TC.NAMES)
def test_case_equals_the_oracle(name):
    got, want = _host(name), TC.expected(name)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        _same(g, w, (name, i))
    if name != 'empty-and-dropped':
        assert all(len(w['idx']) > 0 for w in want)


def test_empty_and_dropped_pictures_leave_zero_rows_or_untouched_rows():
    """count 0 for a picture without candidates and for one whose candidates are all edge-dropped; the host variant returns zero
    rows past the count, the device variant leaves them as they were"""
    pname, pred, tiles, thr, k, keep, m = TC.case('empty-and-dropped')
    tl = _tl(tiles)
    count = np.full(3, -7, np.int32)
    o = [np.full((3, 4), -7, np.float32)] + [np.full((3, 4), -7, np.int32) for _ in range(3)] + [np.full((3, 4, 4), -7, np.int32)]
    check(lib.ssd_detout_tiles(b'vgg300', 2, _lib.device(), np_ptr(pred), C.cast(tiling.tile_structs(tl), C.c_void_p), 4, 3, thr, k, keep, m, 4,
                               np_ptr(count), *[np_ptr(a) for a in o]))
    assert count.tolist() == [0, 0, 1]
    assert all(not a[:2].any() and not a[2, 1:].any() for a in o) and o[0][2, 0] == np.float32(0.7)
    raw = _dev('empty-and-dropped', [4], out_cap=4)
    assert raw['count'].tolist() == [0, 0, 1]
    assert all((raw[k_][:2] == -7).all() and (raw[k_][2, 1:] == -7).all() for k_ in KEYS)
    _same(_rows(raw, 2, 4), TC.expected('empty-and-dropped')[2], 'device')


# ------------------------------------------------------------------------------------------------ 2. the device entry points
@pytest.mark.parametrize('name,splits', [('two-pictures', [10]), ('two-pictures', [3, 5, 2]), ('scene', [4, 3]), ('scene', [1] * 7),
                                         ('rules', [2, 1])])
def test_add_dev_in_parts_equals_one_call(name, splits):
    """a picture's tiles may span calls (here: split in the middle of a picture)"""
    raw = _dev(name, splits)
    want = TC.expected(name)
    keep = TC.case(name)[5]
    for i, w in enumerate(want):
        assert int(raw['count'][i]) == len(w['idx'])
        _same(_rows(raw, i, keep), w, (name, splits, i))


def test_out_cap_below_the_count_clips_the_rows():
    want = TC.expected('two-pictures')
    raw = _dev('two-pictures', [10], out_cap=9)
    for i, w in enumerate(want):
        assert int(raw['count'][i]) == len(w['idx']) > 9
        _same(_rows(raw, i, 9), {k: w[k][:9] for k in w}, i)


def test_two_runs_are_byte_equal():
    a, b = _dev('scene-k8-keep5', [7]), _dev('scene-k8-keep5', [7])
    c, d = _dev('classes-127', [3]), _dev('classes-127', [2, 1])
    for k in a:
        assert a[k].tobytes() == b[k].tobytes() and c[k].tobytes() == d[k].tobytes(), k


# ------------------------------------------------------------------------------------------------ 3. one tile = DetectionOutput
@pytest.mark.parametrize('name', ['softmax-C3', 'sparse', 'cut-ties', 'keep-top-k-2', 'softmax-vgg512-C3'])
def test_one_tile_picture_equals_detection_output_byte_for_byte(name):
    pname, pred, thr, k, keep = DC.case(name)
    b, A, nv = pred.shape
    sizes = [(640, 480), (300, 300), (4000, 3000)][:b]
    tl = [(i, tiling.Tile(0, 0, w, h, 0), (w, h)) for i, (w, h) in enumerate(sizes)]
    want = [np.zeros(b, np.int32), np.zeros((b, keep), np.float32)] + [np.zeros((b, keep), np.int32) for _ in range(2)] + [np.zeros((b, keep, 4), np.int32)]
    check(lib.ssd_detection_output(pname.encode(), nv - 5, _lib.device(), np_ptr(pred), b, thr, k, keep, keep, *[np_ptr(a) for a in want]))
    got = [np.zeros(b, np.int32), np.zeros((b, keep), np.float32)] + [np.zeros((b, keep), np.int32) for _ in range(3)] + [np.zeros((b, keep, 4), np.int32)]
    check(lib.ssd_detout_tiles(pname.encode(), nv - 5, _lib.device(), np_ptr(pred), C.cast(tiling.tile_structs(tl), C.c_void_p), b, b, thr, k, keep, 2,
                               keep, *[np_ptr(a) for a in got]))
    assert want[0].sum() > 0
    for g, w in zip(got[:4] + got[5:], want):
        assert g.tobytes() == w.tobytes()
    assert not got[4].any()


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_come_before_any_launch():
    """every limit is refused on the host with the entry point's name, and nothing is written (tests/test_tiledet_abi.py runs the
    whole list without a GPU)"""
    pname, pred, tiles, thr, k, keep, m = TC.case('rules')
    tl = _tl(tiles)

    def refused(word, tl=tl, ncls=4, n_images=1, thr=thr, k=k, keep=keep, out_cap=4):
        count = np.full(max(n_images, 1), -7, np.int32)
        o = [np.full((1, 4), -7, np.float32)] + [np.full((1, 4), -7, np.int32) for _ in range(3)] + [np.full((1, 4, 4), -7, np.int32)]
        rc = lib.ssd_detout_tiles(b'vgg300', ncls, _lib.device(), np_ptr(pred), C.cast(tiling.tile_structs(tl), C.c_void_p), len(tl), n_images, thr, k,
                                  keep, m, out_cap, np_ptr(count), *[np_ptr(a) for a in o])
        assert rc != 0 and _lib.last_error().startswith('ssd_detout_tiles:') and word in _lib.last_error(), _lib.last_error()
        assert (count == -7).all() and all((a == -7).all() for a in o)

    refused('nms_top_k', k=0)
    refused('nms_top_k', k=1025)
    refused('keep_top_k', keep=0)
    refused('num_classes', ncls=128)
    refused('threshold', thr=-0.1)
    refused('threshold', thr=float('nan'))
    refused('out_cap', out_cap=0)
    refused('ascend', n_images=2)
    refused('leaves', tl=[(0, tiling.Tile(60, 0, 50, 50, 0), (100, 100))] + tl[1:])
    refused('at most 256', tl=[(0, tiling.Tile(0, 0, 10, 10, 0), (10, 10))] * 257)
    with pytest.raises(RuntimeError, match='ssd_detout_tiles: nms_top_k'):
        su.detect_tiles(pred, su.get_preset_by_name(pname), tl, thr, decode='all', nms_top_k=2000)
    (got,) = _host('rules')                                                     # (the same arguments are accepted)
    _same(got, TC.expected('rules')[0], 'accepted')


# ------------------------------------------------------------------------------------------------ 5. the network path
SHAPES = [(700, 1000), (250, 300)]        # (h, w): 7 + 1 tiles at tile 400: two network batches of 4


def test_tiled_detector_decode_all_equals_detect_tiles_on_the_fetched_predictions():
    from ssd_tensorflow_amd.ssdvgg import SSDVGG, Session
    rng = np.random.default_rng(23)
    pics = [rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for h, w in SHAPES]
    with Session(0) as sess:
        net = SSDVGG(sess, 'vgg300')
        net.build_from_vgg(None, 3, max_batch=4, dtype='bf16')
        det = tiling.TiledDetector(net, 400, threshold=0.2, decode='all', nms_top_k=50, keep_top_k=40)
        src = next(tiling.source_batches(pics, len(pics), 0))[:3]
        tiles = det.plan(src[2])
        assert [sum(1 for t in tiles if t[0] == i) for i in range(2)] == [7, 1]
        preds = []
        for x in det.batches(*src):                                            # the very tile batches the detector runs
            preds.append(net.infer(x))
        pred = np.concatenate(preds, 0)
        assert pred.shape == (8, 8732, 8)
        want = su.detect_tiles(pred, net.preset, tiles, 0.2, edge_margin=2, decode='all', nms_top_k=50, keep_top_k=40)
        assert all(len(w['idx']) > 0 for w in want)
        first = det.launch(*src)
        second = det.launch(*src)                                              # before the first is collected: the two output sets
        assert first.out_cap == 40 and first.b == 2
        for ticket in (first, second):
            for i, g in enumerate(ticket.get()):
                _same(g, want[i], ('detector', i))
        # what annotate_batch and DeviceAPCalculator.add_pass read: the device slots of the last pass
        count, conf, cls, box, b, out_cap, _ = second.dev_slots()
        assert (b, out_cap) == (2, 40) and count == second._dev['count'].data_ptr()
        for i, w in enumerate(want):
            n = len(w['idx'])
            assert int(second._dev['count'][i]) == n
            assert np.array_equal(second._dev['cls'][i, :n].cpu().numpy(), w['cls']) and np.array_equal(second._dev['box'][i, :n].cpu().numpy(), w['box'])

