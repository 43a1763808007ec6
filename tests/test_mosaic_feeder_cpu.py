"""CPU half of the mosaic feeder, with the GPU half of a batch replaced by a host stand-in as in
tests/test_feeder_cpu.py: what the workers plan is what the serial generator plans, mosaic=0 changes nothing that travels, the
samples of a mixed batch that are no mosaic keep their draws, and the last epochs of a run carry no mosaic."""
import ctypes as C

import numpy as np
import pytest

import mosaic_ref as mr
from oracle import boxes as ob
from ssd_tensorflow_amd import ssdutils, transforms as T
from ssd_tensorflow_amd.parallel import ShardSampler
from ssd_tensorflow_amd.training_data import TrainingData

W = H = 300
KW = dict(num_train=14, num_valid=5, augment=True, device_tensors=False)


def _prime(preset_name='vgg300'):
    preset = ssdutils.get_preset_by_name(preset_name)
    ssdutils.prime_anchor_table(preset, ob.anchors_abs(ob.anchors(ob.PRESETS[preset_name])))
    return preset


def _host_upload(arrays, gts, slot):
    return {k: np.array(v) for k, v in arrays.items()}, [[tuple(b) for b in g] for g in gts]


def _collect(td, gen, batch, workers):
    td._upload_hook = _host_upload
    return [(x, y, gt) for x, y, gt in gen(batch, workers)]


def _same(a, b):
    assert len(a) == len(b)
    for (xa, ya, ga), (xb, yb, gb) in zip(a, b):
        assert xa.keys() == xb.keys()
        for k in xa:
            assert xa[k].dtype == xb[k].dtype and np.array_equal(xa[k], xb[k]), k
        assert ya == yb and ga == gb


def _structs(arrays):
    n = arrays['params'].size // C.sizeof(T._Params)
    return (T._Params * n).from_buffer_copy(arrays['params'].tobytes())


def test_workers_deliver_the_serial_generators_mosaics():
    _prime()
    td = TrainingData(None, 'vgg300', mosaic=1.0, **KW)
    try:
        td.epoch = 0
        serial = _collect(td, td.train_generator, 4, 0)
        stats = dict(td.feeder_stats)
        two = _collect(td, td.train_generator, 4, 2)
        _same(serial, two)
        assert [len(g) for _, _, g in serial] == [4, 4, 4, 2]
        assert stats['mosaics'] == 14 and stats['cells'] == 56 and td.feeder_stats['mosaics'] == 14 and td.feeder_stats['cells'] == 56
        assert stats['area_fallbacks'] == td.feeder_stats['area_fallbacks']
        recipe = td._recipes['train']
        sampler_idx = [i for idx, _ in ShardSampler(14, 4, 0, 1, td.seed + recipe.salt).batches_with_count(0) for i in idx]
        at = 0
        for arrays, labels, gts in serial:
            b = len(gts)
            cells, src = arrays['cells'], arrays['src_idx']
            assert cells.dtype == np.int32 and cells.shape == (4 * b, 5) and src.shape == (4 * b,)
            p = _structs(arrays)
            assert len(p) == 4 * b
            want_src = recipe.sources(0, sampler_idx[at:at + b])
            for k in range(b):
                quad = cells[4 * k:4 * k + 4]
                assert (quad[:, 0] == k).all()
                mx, my = int(quad[0, 3]), int(quad[0, 4])
                assert [tuple(c) for c in quad[:, 1:]] == mr.layout(mx, my, W, H)
                assert 90 <= mx <= 210 and 90 <= my <= 210
                assert list(src[4 * k:4 * k + 4]) == want_src[k][0] and (mx, my) == want_src[k][1]
                for c in range(4):
                    q = p[4 * k + c]
                    assert not q.expand_on                       # ExpandTransform does not fire in a cell
                    if q.resize_alg == T.INTER_AREA:
                        assert q.crop_w <= 14 * quad[c, 3] and q.crop_h <= 14 * quad[c, 4]
                # the merged boxes: every box lies in (or at least has its centre in) one of the four cells, in cell order
                assert len(gts[k]) >= 1
                order = []
                for bx in gts[k]:
                    cx, cy = bx[2].x * W, bx[2].y * H
                    order.append((0 if cx < mx else 1) + (0 if cy < my else 2))
                assert order == sorted(order), order
            assert arrays['goff'][-1] == sum(len(g) for g in gts)
            at += b
        td.epoch = 1
        other = _collect(td, td.train_generator, 4, 2)
        assert any(not np.array_equal(a[0]['cells'], b[0]['cells']) for a, b in zip(serial, other))
        # validation never mosaics: no new key travels
        valid = _collect(td, td.valid_generator, 4, 0)
        assert all('cells' not in x and 'src_idx' not in x for x, _, _ in valid)
    finally:
        td.close()


def test_mosaic_zero_delivers_the_arrays_of_a_run_without_the_argument():
    _prime()
    plain = TrainingData(None, 'vgg300', **KW)
    zero = TrainingData(None, 'vgg300', mosaic=0.0, mosaic_off_epochs=3, **KW)
    try:
        for workers in (0, 2):
            a = _collect(plain, plain.train_generator, 4, workers)
            b = _collect(zero, zero.train_generator, 4, workers)
            _same(a, b)
            for x, _, _ in b:
                assert 'cells' not in x and 'src_idx' not in x and 'mosaic_stats' not in x
                assert set(x) == {'params', 'packed', 'gt', 'gcls', 'goff'}
        for (xa, _, _), (xb, _, _) in zip(a, b):
            assert all(xa[k].tobytes() == xb[k].tobytes() for k in xa)
        assert zero._recipes['train'].slot_bytes(4) == plain._recipes['train'].slot_bytes(4)
        assert zero.feeder_stats['mosaics'] == 0 and zero.feeder_stats['cells'] == 0
    finally:
        plain.close(); zero.close()


def test_plain_samples_of_a_mixed_batch_keep_their_draws():
    """mosaic=0.5: a sample that is no mosaic is one cell (0, 0, W, H) whose parameter struct is, byte for byte, the one of the
    mosaic=0 run -- but for src_off, the place of its picture among the batch's (more) source pictures -- and whose boxes are
    the same."""
    _prime()
    plain = TrainingData(None, 'vgg300', **KW)
    half = TrainingData(None, 'vgg300', mosaic=0.5, **KW)
    try:
        a = _collect(plain, plain.train_generator, 7, 0)
        b = _collect(half, half.train_generator, 7, 0)
        size = C.sizeof(T._Params)
        off = T._Params.src_off.offset
        n_plain = n_mosaic = 0
        for (xa, ya, ga), (xb, yb, gb) in zip(a, b):
            cells = xb['cells']
            pa, pb = xa['params'].reshape(-1, size).copy(), xb['params'].reshape(-1, size).copy()
            sa, sb = _structs(xa), _structs(xb)
            pa[:, off:off + 8] = 0; pb[:, off:off + 8] = 0
            assert len(ga) == len(gb) == 7
            for k in range(7):
                mine = np.flatnonzero(cells[:, 0] == k)
                if len(mine) == 4:
                    n_mosaic += 1
                    continue
                n_plain += 1
                assert len(mine) == 1 and tuple(cells[mine[0], 1:]) == (0, 0, W, H)
                assert pb[mine[0]].tobytes() == pa[k].tobytes()
                assert ya[k] == yb[k]
                # the picture itself travelled too
                n = sa[k].src_w * sa[k].src_h * 3
                assert np.array_equal(xa['packed'][sa[k].src_off:sa[k].src_off + n], xb['packed'][sb[mine[0]].src_off:sb[mine[0]].src_off + n])
        assert n_plain >= 2 and n_mosaic >= 2
        assert half.feeder_stats['mosaics'] == n_mosaic and half.feeder_stats['cells'] == n_plain + 4 * n_mosaic
    finally:
        plain.close(); half.close()


def test_the_last_epochs_carry_no_mosaic():
    _prime()
    plain = TrainingData(None, 'vgg300', **KW)
    td = TrainingData(None, 'vgg300', mosaic=1.0, mosaic_off_epochs=2, epochs=4, **KW)
    try:
        for e in range(4):
            td.epoch = plain.epoch = e
            got = _collect(td, td.train_generator, 4, 2 if e % 2 else 0)
            if e < 2:
                assert all('cells' in x and x['cells'].shape[0] == 4 * len(g) for x, _, g in got)
            else:
                _same(got, _collect(plain, plain.train_generator, 4, 0))
                assert td.feeder_stats['mosaics'] == 0
    finally:
        plain.close(); td.close()


def test_slots_are_sized_for_four_sources_per_sample():
    _prime()
    plain = TrainingData(None, 'vgg300', **KW)
    td = TrainingData(None, 'vgg300', mosaic=0.25, **KW)
    try:
        r, q = td._recipes['train'], plain._recipes['train']
        assert td.sources_per_batch(r, 8) == 32 and td.sources_per_batch(td._recipes['valid'], 8) == 8
        assert r.slot_bytes(8) - 8192 == 4 * (q.slot_bytes(8) - 8192)
        assert td._recipes['valid'].slot_bytes(8) == plain._recipes['valid'].slot_bytes(8)
    finally:
        plain.close(); td.close()


def test_a_thin_inter_area_cell_falls_back_to_linear():
    """mosaic_cell_resize: INTER_AREA onto a cell that would shrink the frame by more than 14x becomes INTER_LINEAR, counted;
    the draw of the algorithm is the same either way."""
    import random
    from compose_util import sample, test_image
    img = test_image(3, (150, 110))
    resize = T.ResizeTransform(width=96, height=80, algorithms=[T.INTER_AREA])
    for (cw, ch), fell in (((10, 40), 1), ((11, 8), 0), ((96, 7), 1), ((11, 7), 1), ((150, 110), 0)):
        random.seed(1)
        data, _, _, f = T.mosaic_cell_resize(resize, T.ImagePlan(img), None, sample((150, 110)), cw, ch)
        assert f == fell and data.resize == (cw, ch, T.INTER_LINEAR if fell else T.INTER_AREA)
    random.seed(1)
    data, _, _, f = T.mosaic_cell_resize(T.ResizeTransform(width=96, height=80, algorithms=[T.INTER_CUBIC]), T.ImagePlan(img), None,
                                         sample((150, 110)), 1, 1)
    assert f == 0 and data.resize == (1, 1, T.INTER_CUBIC)
