"""GPU: tiled detection -- ssd_merge_tiles through ssdutils.detect_tiles / merge_tile_lists, tiling.TiledDetector and
the drivers' --tile -- against the numpy restatement tests/tiles_ref.py, for exact equality of all five outputs."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import tiles_ref as R
import annotate_ref as AR
from test_annotate import _decode_png
from ssd_tensorflow_amd import _lib, tiling, infer, detect
from ssd_tensorflow_amd import ssdutils as su
from ssd_tensorflow_amd import transforms as T
from ssd_tensorflow_amd import utils as ut
from ssd_tensorflow_amd._lib import lib, np_ptr

pytestmark = pytest.mark.gpu

KEYS = ('conf', 'cls', 'idx', 'tile', 'box')
W, H = 1000, 700
# the kernel's capacity boundaries: tiles per picture, tiles of a picture * tile_cap, candidates sorted in LDS (more: in the workspace)
MERGE_MAX_TILES, MERGE_MAX_CAND, MERGE_LDS_KEYS = tiling.merge_limits()


def _same(got, want, what):
    for k in KEYS:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k, len(got[k]), len(want[k]))


def _tl(image, tiles, size):
    return [(image, tiling.Tile(*t), size) for t in tiles]


@pytest.fixture(scope='module')
def scene():
    return R.planted_scene()


@pytest.fixture(scope='module')
def scene_dets(scene):
    """oracle decode of every tile of the scene, once per (threshold, tile_cap)"""
    pred, tiles, anch = scene
    return {(thr, cap): R.decode_tiles(pred, anch, thr, cap) for thr in (0.3, 0.01) for cap in (1, 50, 200)}


# ------------------------------------------------------------------------------------------------ 1. detect_tiles vs merge_ref
@pytest.mark.parametrize('thr', [0.3, 0.01])
@pytest.mark.parametrize('tile_cap', [1, 50, 200])
def test_detect_tiles_scene(scene, scene_dets, thr, tile_cap):
    pred, tiles, anch = scene
    preset = su.get_preset_by_name('vgg300')
    dets = scene_dets[(thr, tile_cap)]
    seen = set()
    for m in (-1, 0, 2, 40):
        for mo in (None, 5, 200):
            got = su.detect_tiles(pred, preset, _tl(0, tiles, (W, H)), thr, tile_cap, mo, m)
            assert len(got) == 1
            want = R.merge_ref(dets, tiles, (W, H), m, mo)
            _same(got[0], want, (thr, tile_cap, m, mo))
            seen.add(len(want['idx']))
    assert max(seen) > 0 and len(seen) > 1          # the settings differ in what they keep


def test_detect_tiles_two_pictures(scene, scene_dets):
    pred, tiles, anch = scene
    preset = su.get_preset_by_name('vgg300')
    both = np.concatenate([pred, pred[2:3]], 0)
    tl = _tl(0, tiles, (W, H)) + [(1, tiling.Tile(0, 0, 300, 200, 0), (300, 200))]
    got = su.detect_tiles(both, preset, tl, 0.3, 200, 200, 2)
    dets = scene_dets[(0.3, 200)]
    want = R.merge_ref_all(dets + [dets[2]], [(i, tuple(t), s) for i, t, s in tl], 2, 200)
    assert len(got) == 2 and len(want[1]['idx']) > 0
    _same(got[0], want[0], 'picture 0')
    _same(got[1], want[1], 'picture 1')


# ------------------------------------------------------------------------------------------------ 2. identity
def _hot_pred(rng, A, C, n_hot):
    """clusters of confident anchors (neighbours in the anchor order overlap), confidences on a 1/64 grid so that ties occur"""
    pred = np.zeros((A, C + 5), np.float32)
    pred[:, C] = 1
    starts = rng.integers(0, A - 8, n_hot // 4)
    for s in starts:
        c = int(rng.integers(0, C))
        for a in range(s, s + 4):
            pred[a, c] = np.float32(rng.integers(20, 63)) / 64
            pred[a, C + 1:] = rng.normal(0, 0.5, 4).astype(np.float32)
    return pred


@pytest.mark.parametrize('C_', [1, 20, 127])
def test_one_tile_pictures_equal_detect_batch(C_):
    rng = np.random.default_rng(C_)
    preset = su.get_preset_by_name('vgg300')
    pred = np.stack([_hot_pred(rng, 8732, C_, n) for n in (400, 40, 1200)])
    sizes = [(640, 480), (300, 300), (4000, 3000)]
    tl = [(i, tiling.Tile(0, 0, w, h, 0), (w, h)) for i, (w, h) in enumerate(sizes)]
    for thr, cap, mo in ((0.3, 200, 200), (0.5, 50, None), (0.3, 200, 7)):
        got = su.detect_tiles(pred, preset, tl, thr, cap, mo, -1)
        want = su.detect_batch(pred, preset, thr, cap, mo, nms=True)
        assert sum(len(w['idx']) for w in want) > 0
        for g, w_ in zip(got, want):
            for k in ('conf', 'cls', 'idx', 'box'):
                assert g[k].dtype == w_[k].dtype and np.array_equal(g[k], w_[k]), (C_, thr, cap, mo, k)
            assert not g['tile'].any()


# ------------------------------------------------------------------------------------------------ 3. synthetic tile lists
def _grid_tiles(image, nx, ny, side=100):
    """nx * ny windows of side x side pixels that pave a picture"""
    Wp, Hp = nx * side, ny * side
    out = []
    for j in range(ny):
        for i in range(nx):
            interior = (1 if i > 0 else 0) | (2 if i < nx - 1 else 0) | (4 if j > 0 else 0) | (8 if j < ny - 1 else 0)
            out.append((image, tiling.Tile(i * side, j * side, side, side, interior), (Wp, Hp)))
    return out


def _synth(rng, counts, tile_cap, classes, conf_levels, box_lo=80, box_hi=400):
    """tile lists without a prediction tensor: `counts` records claimed per tile (only the first tile_cap exist), boxes random
    on the tile grid, confidences drawn from a few levels (ties within and across tiles), anchors unique inside a tile"""
    n = len(counts)
    count = np.array(counts, np.int32)
    conf = rng.choice(np.array(conf_levels, np.float32), (n, tile_cap)).astype(np.float32)
    cls = rng.choice(np.array(classes, np.int32), (n, tile_cap)).astype(np.int32)
    idx = np.stack([rng.permutation(8732)[:tile_cap] for _ in range(n)]).astype(np.int32) if tile_cap <= 8732 else None
    bw = rng.integers(box_lo, box_hi, (n, tile_cap)); bh = rng.integers(box_lo, box_hi, (n, tile_cap))
    x0 = rng.integers(0, 1000 - bw); y0 = rng.integers(0, 1000 - bh)
    box = np.stack([x0, x0 + bw, y0, y0 + bh], -1).astype(np.int32)
    return count, conf, cls, idx, box


def _synth_ref(tl, lists, tile_cap, m, mo):
    count, conf, cls, idx, box = lists
    dets = []
    for t in range(len(tl)):
        n = min(int(count[t]), tile_cap)
        dets.append(dict(conf=conf[t, :n], cls=cls[t, :n], idx=idx[t, :n], box=box[t, :n]))
    return R.merge_ref_all(dets, [(i, tuple(t), s) for i, t, s in tl], m, mo, tile_cap)


def _run_synth(tl, lists, tile_cap, m, mo, out_cap=None):
    got = su.merge_tile_lists(tl, *lists, tile_cap, mo, m, out_cap=out_cap)
    want = _synth_ref(tl, lists, tile_cap, m, mo)
    assert len(got) == len(want)
    return got, want


LEVELS = [-1.5, -0.25, 0.0, 0.125, 0.5, 0.515625, 0.75]


def test_synthetic_empty_tiles_ties_and_caps():
    rng = np.random.default_rng(11)
    cap = 40
    # picture 0: full, empty, over-full (count > tile_cap) and short tiles; picture 1: every tile empty; picture 2: one tile
    tl = _grid_tiles(0, 3, 2) + _grid_tiles(1, 2, 2) + [(2, tiling.Tile(0, 0, 50, 70, 0), (50, 70))]
    counts = [cap, 0, cap + 37, 3, 0, cap] + [0, 0, 0, 0] + [cap]
    lists = _synth(rng, counts, cap, [0, 126, 5], LEVELS)
    for m, mo in ((-1, None), (2, None), (40, 9), (-1, 0)):
        got, want = _run_synth(tl, lists, cap, m, mo)
        for i in range(3):
            _same(got[i], want[i], (m, mo, i))
        assert len(want[1]['idx']) == 0
    got, want = _run_synth(tl, lists, cap, -1, None)
    c, t = want[0]['conf'], want[0]['tile']
    assert (c < 0).any() and set(want[0]['cls']) == {0, 126, 5}
    assert ((c[1:] == c[:-1]) & (t[1:] != t[:-1])).any()             # exact ties across tiles survived side by side
    # out_cap = 1: one row per picture, count says how many there were
    count = np.full(3, -7, np.int32)
    o = [np.zeros((3, 1), np.float32)] + [np.zeros((3, 1), np.int32) for _ in range(3)] + [np.zeros((3, 1, 4), np.int32)]
    assert lib.ssd_merge_tiles(_lib.device(), C.cast(tiling.tile_structs(tl), C.c_void_p), len(tl), 3, cap, *[np_ptr(a) for a in lists], -1,
                               -1, 1, np_ptr(count), *[np_ptr(a) for a in o]) == 0, _lib.last_error()
    assert list(count) == [len(w['idx']) for w in want]
    for i in (0, 2):
        assert o[0][i, 0] == want[i]['conf'][0] and o[1][i, 0] == want[i]['cls'][0] and o[2][i, 0] == want[i]['idx'][0]
        assert o[3][i, 0] == want[i]['tile'][0] and np.array_equal(o[4][i, 0], want[i]['box'][0])


@pytest.mark.parametrize('classes', [[3, 9, 20], list(range(127))])
def test_synthetic_capacity_boundaries(classes):
    """one candidate fewer than, exactly, and one more than MERGE_LDS_KEYS (the sort moves from LDS to the workspace), few
    classes (segments of more than 64 boxes: the walking NMS) and 127 (segments of at most 64: the in-register NMS)"""
    rng = np.random.default_rng(len(classes))
    cap = 256
    assert MERGE_LDS_KEYS % cap == 0
    full = MERGE_LDS_KEYS // cap
    tl = _grid_tiles(0, full, 1) + _grid_tiles(1, full, 1) + _grid_tiles(2, full + 1, 1) + _grid_tiles(3, 2, 1)
    counts = [cap] * (full - 1) + [cap - 1] + [cap] * full + [cap] * full + [1] + [30, 31]
    lists = _synth(rng, counts, cap, classes, np.arange(-8, 56) / 64.0)
    got, want = _run_synth(tl, lists, cap, -1, None)
    cand = [sum(min(c, cap) for c, t in zip(counts, tl) if t[0] == i) for i in range(4)]
    assert cand == [MERGE_LDS_KEYS - 1, MERGE_LDS_KEYS, MERGE_LDS_KEYS + 1, 61]
    for i in range(4):
        assert 0 < len(want[i]['idx']) <= cand[i] and (i == 3 or len(want[i]['idx']) < cand[i])      # (61 boxes in 127 classes rarely meet)
        _same(got[i], want[i], i)


def test_synthetic_full_capacity():
    """MERGE_MAX_CAND = 128 tiles x 256 records in one picture, beside a small one"""
    rng = np.random.default_rng(128)
    cap = 256
    assert 128 * cap == MERGE_MAX_CAND and 128 <= MERGE_MAX_TILES
    tl = _grid_tiles(0, 16, 8) + _grid_tiles(1, 2, 1)
    lists = _synth(rng, [cap] * 128 + [5, 0], cap, list(range(127)), np.arange(-64, 64) / 128.0, box_lo=150, box_hi=600)
    got, want = _run_synth(tl, lists, cap, -1, 200)
    _same(got[0], want[0], 'full')
    _same(got[1], want[1], 'small')
    assert len(want[0]['idx']) == 200
    got, want = _run_synth(tl, lists, cap, 2, None)
    _same(got[0], want[0], 'full, edge drop')
    assert 200 < len(want[0]['idx']) < MERGE_MAX_CAND


# ------------------------------------------------------------------------------------------------ 4. refusals
def _refused(tl, lists, tile_cap, n_images=None, out_cap=4):
    n_images = (max(t[0] for t in tl) + 1) if n_images is None else n_images
    count = np.full(max(n_images, 1), -7, np.int32)
    g = max(n_images, 1)
    o = [np.full((g, out_cap), -7, np.float32)] + [np.full((g, out_cap), -7, np.int32) for _ in range(3)] + [np.full((g, out_cap, 4), -7, np.int32)]
    rc = lib.ssd_merge_tiles(_lib.device(), C.cast(tiling.tile_structs(tl), C.c_void_p), len(tl), n_images, tile_cap,
                             *[np_ptr(a) for a in lists], 2, -1, out_cap, np_ptr(count), *[np_ptr(a) for a in o])
    assert rc != 0 and 'merge_tiles' in _lib.last_error(), _lib.last_error()
    assert (count == -7).all() and all((a == -7).all() for a in o)             # nothing was written
    return _lib.last_error()


def test_refusals():
    rng = np.random.default_rng(4)
    ok = _grid_tiles(0, 2, 1)
    lists = _synth(rng, [2, 2], 2, [1], LEVELS)
    got, want = _run_synth(ok, lists, 2, 2, None)                              # (the same arguments are accepted)
    _same(got[0], want[0], 'accepted')
    # one tile more than MERGE_MAX_TILES in a picture
    many = [(0, tiling.Tile(0, 0, 10, 10, 0), (10, 10))] * (MERGE_MAX_TILES + 1)
    assert 'tiles' in _refused(many, _synth(rng, [1] * len(many), 1, [1], LEVELS), 1)
    _run_synth(many[:-1], _synth(rng, [1] * MERGE_MAX_TILES, 1, [1], LEVELS), 1, 2, None)
    # tiles of a picture * tile_cap beyond MERGE_MAX_CAND
    assert 'candidates' in _refused(_grid_tiles(0, 5, 1), _synth(rng, [1] * 5, MERGE_MAX_CAND // 4, [1], LEVELS), MERGE_MAX_CAND // 4)
    # tile_cap = 0
    zero = (lists[0], np.zeros((2, 1), np.float32), np.zeros((2, 1), np.int32), np.zeros((2, 1), np.int32), np.zeros((2, 1, 4), np.int32))
    assert 'tile_cap' in _refused(ok, zero, 0)
    with pytest.raises(ValueError, match='merge_tiles'):
        su.detect_tiles(np.zeros((2, 8732, 6), np.float32), su.get_preset_by_name('vgg300'), ok, 0.5, tile_cap=0)
    # image indices not ascending / with a gap / not from 0
    back = [(1, ok[0][1], ok[0][2]), (0, ok[1][1], ok[1][2])]
    assert 'ascend' in _refused(back, lists, 2, n_images=2)
    gap = [(0, ok[0][1], ok[0][2]), (2, ok[1][1], ok[1][2])]
    assert 'ascend' in _refused(gap, lists, 2, n_images=3)
    # a class id of 127
    bad = [a.copy() for a in lists]
    bad[2][1, 1] = 127
    assert 'class' in _refused(ok, bad, 2)
    # out_cap = 0, a tile that leaves its picture
    assert 'out_cap' in _refused(ok, lists, 2, out_cap=0)
    out = [(0, tiling.Tile(60, 0, 50, 50, 0), (100, 100))]
    assert 'leaves' in _refused(out, _synth(rng, [1], 2, [1], LEVELS), 2)


# ------------------------------------------------------------------------------------------------ 5. - 7. the network path
SHAPES = [(700, 1000), (250, 300), (1000, 700)]        # (h, w): 7 + 1 + 7 tiles at tile 400, overlap 0.25


@pytest.fixture(scope='module')
def pictures(tmp_path_factory):
    d = tmp_path_factory.mktemp('tiles')
    rng = np.random.default_rng(21)
    files = []
    for k, (h, w) in enumerate(SHAPES):
        p = str(d / ('pic%d.npy' % k))
        np.save(p, rng.integers(0, 256, (h, w, 3)).astype(np.uint8))
        files.append(p)
    return files


@pytest.fixture(scope='module')
def model(tmp_path_factory):
    """a one-class checkpoint on Xavier weights: its confidences scatter around 0.5, the drivers' fixed threshold"""
    from ssd_tensorflow_amd.ssdvgg import SSDVGG, Session
    d = tmp_path_factory.mktemp('run')
    path = str(d / 'final.npz')
    with Session(0) as sess:
        net = SSDVGG(sess, 'vgg300')
        net.build_from_vgg(None, 1, max_batch=2)
        net.build_optimizer()
        net.save_checkpoint(path, class_names=['thing'])
    return path


def _net(sess, model, max_batch=4):
    from ssd_tensorflow_amd.ssdvgg import SSDVGG
    net = SSDVGG(sess, su.get_preset_by_name('vgg300'))
    net.build_from_metagraph(None, model, max_batch=max_batch)
    return net


def _sources(files):
    return next(tiling.source_batches(files, len(files), 0))[:3]


def _tile_dets(net, det, src, thr, cap):
    """the nms=False detections of the very tile batches the detector runs, through net.infer_dev + detect_last"""
    out = []
    for x in det.batches(*src):
        net.infer_dev(x)
        out += net.detect_last(x.shape[0], thr, cap, None, nms=False)
    return out


def _expect(net, det, src, thr, cap=200, m=2, mo=200):
    tl = [(i, tuple(t), s) for i, t, s in det.plan(src[2])]
    return R.merge_ref_all(_tile_dets(net, det, src, thr, cap), tl, m, mo)


def test_tile_tensors_equal_crops(pictures, model):
    from ssd_tensorflow_amd.ssdvgg import Session
    img = np.load(pictures[0])
    assert img.shape == (700, 1000, 3) and img.dtype == np.uint8
    with Session(0) as sess:
        net = _net(sess, model)
        det = tiling.TiledDetector(net, 400)
        src = _sources(pictures[:1])
        tiles = det.plan(src[2])
        assert len(tiles) == 7
        got = torch.cat(list(det.batches(*src)), 0)
        plans = []
        for _, t, _ in tiles:
            plan = T.ImagePlan(np.ascontiguousarray(img[t.y0:t.y0 + t.h, t.x0:t.x0 + t.w]))      # the crop as a picture of its own
            plan.resize = (300, 300, T.INTER_LINEAR)
            plans.append(plan)
        want = T.augment_batch(plans, 300, 300)
        assert got.shape == want.shape == (7, 300, 300, 3)
        for k in range(7):
            assert torch.equal(got[k], want[k]), tiles[k]


def test_tiled_detector_end_to_end(pictures, model):
    from ssd_tensorflow_amd.ssdvgg import Session
    with Session(0) as sess:
        net = _net(sess, model, max_batch=4)
        det = tiling.TiledDetector(net, 400, threshold=0.5)
        src = _sources(pictures)
        assert [sum(1 for t in det.plan(src[2]) if t[0] == i) for i in range(3)] == [7, 1, 7]
        back = _sources(pictures[::-1])
        want = _expect(net, det, src, 0.5)
        want_back = _expect(net, det, back, 0.5)
        assert all(len(w['idx']) > 0 for w in want)
        first = det.launch(*src)
        second = det.launch(*back)                      # before the first is collected
        assert first.out_cap == 200 and first.b == 3
        got = first.get()
        got_back = second.get()
        for i in range(3):
            _same(got[i], want[i], i)
            _same(got_back[i], want_back[i], ('second', i))
            _same(got_back[2 - i], want[i], ('reversed', i))
        # the device arrays the drawing reads hold the same detections
        for i, w in enumerate(want_back):
            n = len(w['idx'])
            assert int(second._dev['count'][i]) == n and second.count_dev == second._dev['count'].data_ptr()
            assert np.array_equal(second._dev['cls'][i, :n].cpu().numpy(), w['cls']) and np.array_equal(second._dev['box'][i, :n].cpu().numpy(), w['box'])
        third = det.launch(*src)
        with pytest.raises(RuntimeError, match='overwritten'):
            first.get()
        for i, g in enumerate(third.get()):
            _same(g, want[i], ('third', i))


def _txt(det, names):
    return ['{} {} {} {} {} {}\n'.format(b.label, b.labelid, b.center.x, b.center.y, b.size.w, b.size.h)
            for _, b in su.boxes_from_detection(det, dict(enumerate(names)))]


def _drawn(path, det, names, colors):
    img = np.load(path)
    h, w = img.shape[:2]
    px = [AR.rect1000(b, w, h) for b in det['box']]
    return AR.draw(img, AR.style_boxes(px, det['cls'], colors, names))


def _tree(d):
    return {f: open(os.path.join(d, f), 'rb').read() for f in sorted(os.listdir(d))}


def test_drivers_tile(pictures, model, tmp_path, capsys):
    from ssd_tensorflow_amd.ssdvgg import Session
    names = ['thing']
    colors = [ut.default_colors(names)[n] for n in names]
    with Session(0) as sess:
        net = _net(sess, model, max_batch=4)
        det = tiling.TiledDetector(net, 400, threshold=0.5)
        want = [{k: v.copy() for k, v in d.items()} for d in det.launch(*_sources(pictures)).get()]
    assert all(len(w['idx']) > 0 for w in want)
    # detect.py: the .txt files and the pictures
    odir = str(tmp_path / 'detect')
    assert detect.main(['--model', model, '--output-dir', odir, '--batch-size', '4', '--tile', '400'] + pictures) == 0
    for f, w in zip(pictures, want):
        base = os.path.join(odir, os.path.basename(f))
        assert open(base + '.txt').readlines() == _txt(w, names)
        got = _decode_png(open(base + '.png', 'rb').read())[:, :, ::-1]
        assert np.array_equal(got, _drawn(f, w, names, colors))
    # infer.py --annotate: the pictures and the count it reports; two pictures per launch, so the passes overlap
    capsys.readouterr()
    odir = str(tmp_path / 'infer')
    common = ['--name', os.path.dirname(model), '--threshold', '0.5', '--batch-size', '4']
    assert infer.main(common + ['--tile', '400', '--annotate', 'true', '--pascal-summary', 'true', '--output-dir', odir] + pictures) == 0
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith('[i] Processed')]
    assert line == ['[i] Processed 3 images, %d detections' % sum(len(w['idx']) for w in want)]
    for f, w in zip(pictures, want):
        got = _decode_png(open(os.path.join(odir, os.path.basename(f) + '.png'), 'rb').read())[:, :, ::-1]
        assert np.array_equal(got, _drawn(f, w, names, colors))
    from ssd_tensorflow_amd.pascal_summary import PascalSummary
    summary = PascalSummary()
    for f, w in zip(pictures, want):
        h_, w_ = np.load(f, mmap_mode='r').shape[:2]
        summary.add_detections(f, su.boxes_from_detection(w, dict(enumerate(names))), img_size=ut.Size(w_, h_))
    os.makedirs(str(tmp_path / 'summary'))
    summary.write_summary(str(tmp_path / 'summary'))
    assert _tree(str(tmp_path / 'summary')) == {k: v for k, v in _tree(odir).items() if k.startswith('comp4_')} != {}


def test_drivers_tile_zero_is_untiled(pictures, model, tmp_path, capsys):
    flags = ['--tile', '0', '--tile-overlap', '0.5', '--tile-whole', 'false', '--tile-edge-margin', '7']
    a, b = str(tmp_path / 'd0'), str(tmp_path / 'd1')
    assert detect.main(['--model', model, '--output-dir', a, '--batch-size', '2'] + pictures) == 0
    assert detect.main(['--model', model, '--output-dir', b, '--batch-size', '2'] + flags + pictures) == 0
    ta, tb = _tree(a), _tree(b)
    assert len(ta) == 6 and ta == tb and any(len(v) > 0 for k, v in ta.items() if k.endswith('.txt'))
    a, b = str(tmp_path / 'i0'), str(tmp_path / 'i1')
    common = ['--name', os.path.dirname(model), '--threshold', '0.5', '--batch-size', '2', '--annotate', 'true', '--pascal-summary', 'true']
    capsys.readouterr()
    assert infer.main(common + ['--output-dir', a] + pictures) == 0
    out_a = [l for l in capsys.readouterr().out.splitlines() if l.startswith('[i] Processed')]
    assert infer.main(common + ['--output-dir', b] + flags + pictures) == 0
    out_b = [l for l in capsys.readouterr().out.splitlines() if l.startswith('[i] Processed')]
    ta, tb = _tree(a), _tree(b)
    assert out_a == out_b and len(out_a) == 1 and len(ta) >= 3 and ta == tb
