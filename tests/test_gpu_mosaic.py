"""-m gpu, DESIGN.md 39: the cells entry of the augmentation (ssd_augment_cells_dev) and the mosaic feeder on the device.

The contract of a cell is "bit for bit what ssd_augment_batch_dev writes for the same struct with out_w = w, out_h = h", so
the reference of every pixel comparison is the sibling entry on the same plan (np.array_equal); placement is judged apart
from the GPU by a case without resize arithmetic against the oracle's pixel operations and tests/mosaic_ref.compose.
The output sample is 96 x 80; the sources are 150 x 110, 97 x 61, 64 x 64 and 200 x 33."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import compose_util as cu
import mosaic_ref as mr
from ssd_tensorflow_amd import transforms as T
from ssd_tensorflow_amd._lib import lib, check
from ssd_tensorflow_amd.utils import Size

pytestmark = pytest.mark.gpu

W, H = 96, 80
SIZES = [(150, 110), (97, 61), (64, 64), (200, 33)]
CENTRES = [(48, 40), (1, 1), (95, 79), (37, 53)]
WIN = dict(window=(0.15, 0.85, 0.2, 0.9))
ALGS = [T.INTER_NEAREST, T.INTER_LINEAR, T.INTER_CUBIC, T.INTER_AREA, T.INTER_LANCZOS4]


def _lists(rs):
    """step lists that end in (or hold) the resize `rs`: the uint8 path with the photometric pre-pass, a crop and a flip; the
    float (expanded) path; steps and a flip behind the resize; a bare channel reorder; a canvas made uint8 again"""
    return [[('brightness', {}), ('contrast', {}), ('hue', {}), ('crop', WIN), ('flip', {}), rs],
            [('expand', {}), ('crop', WIN), rs],
            [rs, ('contrast', {}), ('hue', {}), ('flip', {}), ('brightness', {})],
            [('reorder', {}), rs],
            [('expand', {}), ('brightness', {}), ('flip', {}), rs, ('saturation', {})],
            [('saturation', {}), ('crop', WIN), ('hue', {}), rs, ('flip', {})]]


def _cell_plan(img, cell, alg, which, seed):
    """the plan of list `which` resized to the cell by `alg`; INTER_AREA that would shrink by more than the tap table's 14x
    becomes INTER_LINEAR, as the feeder's planner does"""
    cw, ch = cell[2], cell[3]
    for a in (alg, T.INTER_LINEAR):
        plan, _ = cu.compose_mirror(_lists(('resize', dict(size=(cw, ch), algorithms=[a])))[which], img, seed)
        frame = plan.size
        if a != T.INTER_AREA or (frame.w <= 14 * cw and frame.h <= 14 * ch):
            return plan
    raise AssertionError


@pytest.fixture(scope='module')
def images():
    return [cu.test_image(700 + i, s) for i, s in enumerate(SIZES)]


@pytest.fixture(scope='module')
def mosaics(images):
    """20 mosaics: every centre five times, the algorithm and the step list of a cell rotating so that each of the five
    algorithms meets each kind of list and each kind of cell (one pixel, one row, one column, widths that are no multiple of 64).
    -> plans, cells [80][5], the kernel's samples [20][80][96][3], per cell the sibling entry's output"""
    plans, cells, algs = [], [], set()
    for s, (centre, r) in enumerate((c, r) for c in CENTRES for r in range(5)):
        for c, cell in enumerate(mr.layout(centre[0], centre[1], W, H)):
            plan = _cell_plan(images[(c + r) % 4], (0, 0, cell[2], cell[3]), ALGS[(c + r) % 5], (c + 2 * r + s) % 6, 4000 + 10 * s + c)
            plans.append(plan); cells.append((s,) + cell); algs.add((plan.resize[2], plan.is_float_at_resize))
    assert {a for a, _ in algs} == set(ALGS) and {f for _, f in algs} == {True, False}
    got = T.augment_cells(plans, cells, 20, W, H).cpu().numpy()
    alone = [T.augment_batch([p], c[3], c[4]).cpu().numpy()[0] for p, c in zip(plans, cells)]
    return plans, np.array(cells, np.int32), got, alone


def test_every_cell_equals_the_batch_entry_on_the_same_plan(mosaics):
    plans, cells, got, alone = mosaics
    seen = set()
    for i, (p, (s, x0, y0, w, h)) in enumerate(zip(plans, cells)):
        assert alone[i].shape == (h, w, 3)
        part = got[s, y0:y0 + h, x0:x0 + w]
        assert np.array_equal(part, alone[i]), 'cell %d (%d x %d at %d, %d of sample %d, alg %d): max diff %g' % (
            i, w, h, x0, y0, s, p.resize[2], np.abs(part - alone[i]).max())
        seen.add((p.resize[2], bool(p.is_float_at_resize), p.crop is not None, bool(p.flip), bool(p.post), bool(p.out_flip)))
    # what the rotation covered: each algorithm on the uint8 and on the float path; crops, flips, post steps, output flips
    for alg in ALGS:
        assert any(k[0] == alg and k[1] for k in seen) and any(k[0] == alg and not k[1] for k in seen), alg
    assert any(k[2] for k in seen) and any(k[3] for k in seen) and any(k[4] for k in seen) and any(k[5] for k in seen)
    assert {(1, 1), (95, 1), (1, 79), (37, 53), (59, 27), (48, 40)} <= {(int(c[3]), int(c[4])) for c in cells}
    assert np.isfinite(got).all()
    assert np.array_equal(got, mr.compose(alone, cells, W, H, 20))


def test_placement_without_resize_arithmetic_against_the_oracle(images):
    """Same-size NEAREST: each cell is a crop of its picture of exactly the cell's size, behind the whole photometric chain and a
    flip -- exact integer pixels on both sides, so the composition is judged by the oracle's pixel operations and
    mosaic_ref.compose, not by a GPU kernel.  Centre (37, 53): cell widths 37 and 59, the 27-row cells fit the 200 x 33 source."""
    cells = [(0,) + c for c in mr.layout(37, 53, W, H)]
    plans = []
    for c, (img, cell) in enumerate(zip(images, cells)):
        cw, ch = cell[3], cell[4]
        random.seed(8800 + c)
        args = (T.ImagePlan(img), None, cu.sample((img.shape[1], img.shape[0])))
        for st in [('brightness', {}), ('contrast', {}), ('saturation', {}), ('hue', {}), ('reorder', {})]:
            args = cu.mirror_step(st, args)
        x0, y0 = 3 + c, 1 + c
        args = T.SamplerTransform(sample=True).crop(*args, np.array([x0, x0 + cw, y0, y0 + ch]))
        if c % 2:
            args = cu.mirror_step(('flip', {}), args)
        args = cu.mirror_step(('resize', dict(size=(cw, ch), algorithms=[T.INTER_NEAREST])), args)
        assert args[0].crop[2:] == (cw, ch)
        plans.append(args[0])
    want = mr.compose([cu.run_plan(p) for p in plans], cells, W, H)
    got = T.augment_cells(plans, cells, 1, W, H).cpu().numpy()
    assert np.array_equal(got, want), np.abs(got - want).max()


def test_a_whole_sample_cell_between_two_mosaics_equals_the_batch_entry(images):
    plans, cells = [], []
    for s, centre in ((0, (37, 53)), (2, (48, 40))):
        for c, cell in enumerate(mr.layout(centre[0], centre[1], W, H)):
            plans.append(_cell_plan(images[c], (0, 0, cell[2], cell[3]), ALGS[(c + s) % 5], c, 5200 + 10 * s + c)); cells.append((s,) + cell)
    whole = _cell_plan(images[0], (0, 0, W, H), T.INTER_CUBIC, 0, 5300)
    plans.insert(4, whole); cells.insert(4, (1, 0, 0, W, H))
    got = T.augment_cells(plans, cells, 3, W, H).cpu().numpy()
    want = T.augment_batch([whole], W, H).cpu().numpy()
    assert np.array_equal(got[1], want[0])
    # and a batch of whole-sample cells alone is the batch entry's batch
    five = [_cell_plan(images[i % 4], (0, 0, W, H), ALGS[i], i, 5400 + i) for i in range(5)]
    assert np.array_equal(T.augment_cells(five, [(i, 0, 0, W, H) for i in range(5)], 5, W, H).cpu().numpy(),
                          T.augment_batch(five, W, H).cpu().numpy())


def test_every_pixel_is_written_and_nothing_outside(mosaics):
    """out_dev full of NaN inside a larger buffer whose margins hold a sentinel: no NaN remains, the margins are untouched."""
    plans, cells, want, _ = mosaics
    margin, n = 4096, 20 * H * W * 3
    big = torch.full((n + 2 * margin,), -7777.0, dtype=torch.float32, device='cuda')
    out = big[margin:margin + n].view(20, H, W, 3)
    out.fill_(float('nan'))
    got = T.augment_cells(plans, cells, 20, W, H, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    host = big.cpu().numpy()
    assert (host[:margin] == -7777.0).all() and (host[margin + n:] == -7777.0).all()
    assert not np.isnan(host).any()
    assert np.array_equal(host[margin:margin + n].reshape(20, H, W, 3), want)


def test_refusals_reach_python_as_errors(images):
    plans = [_cell_plan(images[c], (0, 0, 48, 40), T.INTER_LINEAR, 3, 1) for c in range(4)]
    cells = [(0, 0, 0, 48, 40), (0, 47, 0, 48, 40), (0, 0, 40, 48, 40), (0, 48, 40, 48, 40)]
    with pytest.raises(RuntimeError, match='overlap'):
        T.augment_cells(plans, cells, 1, W, H)
    with pytest.raises(ValueError, match='its cell'):
        T.augment_cells(plans, [(0,) + c for c in mr.layout(37, 53, W, H)], 1, W, H)


# ---- the feeder ---------------------------------------------------------------------------------------------------------
def _capture(td, batch, workers=0):
    """what travels: the arrays and merged boxes of an epoch's batches (host copies), without touching the GPU"""
    keep = []
    td._upload_hook = lambda arrays, gts, slot: ({k: np.array(v) for k, v in arrays.items()}, list(gts))
    try:
        for x, y, gt in td.train_generator(batch, workers):
            keep.append((x, gt))
    finally:
        td._upload_hook = None
    return keep


def _cells_alone(arrays, Wp, Hp):
    """every source picture of a batch through ssd_augment_batch_dev alone, at its cell's size"""
    size = C.sizeof(T._Params)
    packed = torch.from_numpy(arrays['packed']).cuda()
    outs = []
    for i, (_, _, _, cw, ch) in enumerate(arrays['cells']):
        one = np.ascontiguousarray(arrays['params'][i * size:(i + 1) * size])
        out = torch.empty((1, ch, cw, 3), dtype=torch.float32, device='cuda')
        ws = torch.empty((lib.ssd_augment_ws_bytes(1, int(cw), int(ch)),), dtype=torch.uint8, device='cuda')
        check(lib.ssd_augment_batch_dev(packed.data_ptr(), C.c_void_p(one.ctypes.data), 1, int(cw), int(ch), out.data_ptr(), ws.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream))
        outs.append(out.cpu().numpy()[0])
    return outs


def test_training_data_mosaics_on_the_device():
    from ssd_tensorflow_amd.ssdutils import encode_labels_batch
    from ssd_tensorflow_amd.ssdvgg import SSDVGG, Session
    from ssd_tensorflow_amd.training_data import TrainingData, _gt_arrays
    random.seed(5)
    td = TrainingData(None, 'vgg300', num_train=7, num_valid=3, augment=True, mosaic=1.0)
    try:
        travelled = _capture(td, 3)
        serial = [(x.clone(), y.clone(), gt) for x, y, gt in td.train_generator(3)]
        assert td.feeder_stats['mosaics'] == 7 and td.feeder_stats['cells'] == 28
        assert [x.shape[0] for x, _, _ in serial] == [3, 3, 1]
        for (arrays, gts), (x, y, gt) in zip(travelled, serial):
            b = len(gts)
            assert tuple(x.shape) == (b, 300, 300, 3) and tuple(y.shape) == (b, 8732, 25) and gt == gts
            assert arrays['cells'].shape == (4 * b, 5)
            want = mr.compose(_cells_alone(arrays, 300, 300), arrays['cells'], 300, 300, b)
            assert np.array_equal(x.cpu().numpy(), want)
            bxs, cls = _gt_arrays(gt)
            lab = encode_labels_batch(td.preset, 20, bxs, cls)
            got = y.cpu().numpy()
            assert np.array_equal(got[:, :, :21], lab[:, :, :21]) and np.allclose(got[:, :, 21:], lab[:, :, 21:], rtol=2e-7, atol=1e-7)
            assert all(int((got[k][:, 20] != 0).sum()) < 8732 for k in range(b))          # a positive anchor in every sample
        two = [(x.clone(), y.clone(), gt) for x, y, gt in td.train_generator(3, 2)]
        assert len(two) == len(serial)
        for (xa, ya, ga), (xb, yb, gb) in zip(serial, two):
            assert torch.equal(xa, xb) and torch.equal(ya, yb) and ga == gb
        assert td.feeder_stats['mosaics'] == 7 and td.feeder_stats['cells'] == 28
        sess = Session(0)
        net = SSDVGG(sess, td.preset)
        net.build_from_vgg(None, 20, max_batch=3)
        net.build_optimizer(learning_rate=1e-4)
        x, y, _ = serial[0]
        res, L, _ = sess.run([net.result, net.losses, net.optimizer], feed_dict={net.image_input: x, net.labels: y})
        assert res.shape == tuple(y.shape) and np.isfinite(L['total'])
        sess.close()
    finally:
        td.close()


def test_mosaics_from_jpegs_decoded_on_the_gpu_and_cached(tmp_path):
    """decoder='gpu' with a small arena: a mosaic's four source pictures are decoded (or found in HBM) one by one; both epochs
    equal the pixel path's batches bit for bit, and from the first partner that was seen before on the cache serves."""
    import source_jpegset as js
    from ssd_tensorflow_amd.training_data import TrainingData
    images = js.write_dataset(tmp_path, js.ok_files(js.golden())[:14], 4)
    kw = dict(data_source='jpegset', mosaic=1.0)

    def drain(td, epoch, workers):
        td.epoch = epoch
        return [(x.clone(), y.clone(), gt) for x, y, gt in td.train_generator(4, workers)]

    ref = TrainingData(str(tmp_path), 'vgg300', images=images, **kw)
    try:
        want = {e: drain(ref, e, 0) for e in (0, 1)}
    finally:
        ref.close()
    td = TrainingData(str(tmp_path), 'vgg300', decoder='gpu', cache_bytes=3 << 20, **kw)
    try:
        for e, workers in ((0, 0), (1, 2)):
            got = drain(td, e, workers)
            assert len(got) == len(want[e])
            for (xa, ya, ga), (xb, yb, gb) in zip(want[e], got):
                assert torch.equal(xa, xb) and torch.equal(ya, yb) and ga == gb
            st = td.feeder_stats
            assert st['mosaics'] == 10 and st['cells'] == 40
            assert st['decoded'] + st['fallbacks'] + st['cache_hits'] == 40
        assert td.feeder_stats['cache_hits'] > 0
        assert 0 < td._arena.used <= 3 << 20
    finally:
        td.close()
