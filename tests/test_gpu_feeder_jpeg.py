"""-m gpu, DESIGN.md 17: training fed from JPEG files that are decoded on the GPU (decoder='gpu') and kept in HBM (cache_bytes).
The reference of every comparison is the existing pixel path -- the same TrainingData with images={filename: libjpeg-turbo's
pixels} and the default decoder: `images` and `labels` of every batch must equal its tensors bit for bit, whatever decoded the
pictures, wherever they lie and whichever process planned the batch."""
import os

import numpy as np
import pytest
import torch

import source_jpegset as js
from ssd_tensorflow_amd import train
from ssd_tensorflow_amd.parallel import ShardSampler
from ssd_tensorflow_amd.training_data import TrainingData

pytestmark = pytest.mark.gpu

BATCH = 4
NUM_VALID = 8


def _td(root, **kw):
    return TrainingData(str(root), 'vgg300', data_source='jpegset', **kw)


def _drain(td, which, workers, epoch):
    td.epoch = epoch
    gen = td.train_generator if which == 'train' else td.valid_generator
    return [(x.clone(), y.clone(), gt) for x, y, gt in gen(BATCH, workers)]


def _equal(want, got):
    assert len(want) == len(got)
    for (xa, ya, ga), (xb, yb, gb) in zip(want, got):
        assert torch.equal(xa, xb) and torch.equal(ya, yb) and ga == gb


def _reference(root, images):
    td = _td(root, images=images)
    try:
        return {(which, epoch): _drain(td, which, 0, epoch) for which in ('train', 'valid') for epoch in (0, 1)}
    finally:
        td.close()


@pytest.fixture(scope='module')
def jpegset(tmp_path_factory):
    """28 JPEGs (20 train, 8 valid) and the pixel path's batches of two epochs of both"""
    root = tmp_path_factory.mktemp('jpegset')
    images = js.write_dataset(root, js.ok_files(js.golden())[:28], NUM_VALID)
    return root, images, _reference(root, images)


@pytest.mark.parametrize('workers', [0, 2])
def test_batches_equal_the_pixel_paths(jpegset, workers):
    root, _, ref = jpegset
    td = _td(root, decoder='gpu')
    try:
        for epoch in (0, 1):
            _equal(ref['train', epoch], _drain(td, 'train', workers, epoch))
            assert td.feeder_stats['decoded'] == td.num_train and td.feeder_stats['fallbacks'] == td.feeder_stats['cache_hits'] == 0
            _equal(ref['valid', epoch], _drain(td, 'valid', workers, epoch))
    finally:
        td.close()


@pytest.mark.parametrize('cache_bytes', [0, 4 << 20])
@pytest.mark.parametrize('unsupported', [False, True])
def test_mixed_sources_in_one_batch(tmp_path, unsupported, cache_bytes):
    """A .npy array and (with Pillow) a progressive JPEG among the JPEGs: their pixels travel as today and are copied behind the
    decoded pictures, or into the arena."""
    z = js.golden()
    files = js.ok_files(z)[28:40]
    files.insert(2, ('array', np.random.default_rng(5).integers(0, 256, (37, 52, 3), dtype=np.uint8), None))
    if unsupported:
        Image = pytest.importorskip('PIL.Image')
        import io
        data = z['unsup_0_jpg'].tobytes()
        with Image.open(io.BytesIO(data)) as im:
            pixels = np.ascontiguousarray(np.asarray(im.convert('RGB'))[:, :, ::-1])
        files.insert(5, ('progressive', data, pixels))
    images = js.write_dataset(tmp_path, files, 4)
    ref = _reference(tmp_path, images)
    td = _td(tmp_path, decoder='gpu', cache_bytes=cache_bytes)
    try:
        for epoch in (0, 1):
            _equal(ref['train', epoch], _drain(td, 'train', 2, epoch))
            st = td.feeder_stats
            n_fall = sum(('array' in s.filename or 'progressive' in s.filename) for s in td.train_samples)
            assert n_fall == 1 + int(unsupported)
            if cache_bytes and epoch:
                assert (st['decoded'], st['fallbacks'], st['cache_hits']) == (0, 0, td.num_train)
            else:
                assert (st['decoded'], st['fallbacks'], st['cache_hits']) == (td.num_train - n_fall, n_fall, 0)
        _equal(ref['valid', 1], _drain(td, 'valid', 0, 1))
    finally:
        td.close()


def test_a_batch_larger_than_its_slot_takes_the_serial_upload(jpegset):
    root, _, ref = jpegset
    td = _td(root, decoder='gpu')
    try:
        td._max_image_bytes, td._max_coef_bytes = 16000, 0       # the host slots shrink; the device scratch keeps its size
        _equal(ref['train', 0], _drain(td, 'train', 2, 0))
        recipe = td._recipes['train']
        batches = ShardSampler(recipe.total, BATCH, td.rank, td.world, td.seed + recipe.salt).batches_with_count(0)
        sizes = [sum(v.nbytes for v in recipe.plan(0, idx)[0].values()) for idx, _ in batches]
        assert max(sizes) > recipe.pool.slot_bytes > min(sizes)  # some batches came through the pipe, some in their slot
    finally:
        td.close()


@pytest.mark.parametrize('workers', [(2, 2), (0, 0), (2, 0)])
def test_cached_epoch_needs_no_file(tmp_path, jpegset, workers):
    """Room for every picture: the second epoch is served from HBM -- the files are gone by then.  (2, 0): the entries were
    appended on the feeder's stream and are read by the serial generator on the caller's."""
    _, _, ref = jpegset
    files = js.ok_files(js.golden())[:28]
    js.write_dataset(tmp_path, files, NUM_VALID)
    td = _td(tmp_path, decoder='gpu', cache_bytes=2 << 20)
    try:
        _equal(ref['train', 0], _drain(td, 'train', workers[0], 0))
        assert td.feeder_stats['decoded'] == td.num_train and td.feeder_stats['cache_hits'] == 0
        for s in td.train_samples:
            os.remove(s.filename)
        _equal(ref['train', 1], _drain(td, 'train', workers[1], 1))
        assert td.feeder_stats['cache_hits'] == td.num_train and td.feeder_stats['decoded'] == td.feeder_stats['fallbacks'] == 0
    finally:
        td.close()


def test_a_full_arena_overflows_into_scratch(jpegset):
    """Room for about one and a half batches: the rest of every epoch is decoded into the device slots' scratch, which is reused
    batch after batch behind the consumer's release."""
    root, images, ref = jpegset
    td = _td(root, decoder='gpu', cache_bytes=int(1.5 * BATCH * np.mean([v.nbytes for v in images.values()])))
    try:
        for epoch in (0, 1):
            _equal(ref['train', epoch], _drain(td, 'train', 2, epoch))
        st = td.feeder_stats
        assert 0 < st['cache_hits'] <= len(td._arena.table) < td.num_train and st['decoded'] == td.num_train - st['cache_hits']
        assert td._arena.used <= td._arena.cache_bytes
    finally:
        td.close()


def test_train_and_valid_generators_share_the_arena(jpegset):
    root, _, ref = jpegset
    td = _td(root, decoder='gpu', cache_bytes=2 << 20)
    try:
        for epoch in (0, 1):
            td.epoch = epoch
            gt_, gv_ = td.train_generator(BATCH, 2), td.valid_generator(BATCH, 2)
            t_mixed, v_mixed = [], []
            for k in range(5):
                x, y, g = next(gt_)
                if k < 2:
                    xv, yv, gv = next(gv_)
                    v_mixed.append((xv.clone(), yv.clone(), gv))
                t_mixed.append((x.clone(), y.clone(), g))
            _equal(ref['train', epoch], t_mixed)
            _equal(ref['valid', epoch], v_mixed)
            gt_.close(); gv_.close()
        assert len(td._arena.table) == td.num_train + td.num_valid
    finally:
        td.close()


def test_train_driver_with_the_gpu_decoder_matches_pillow(tmp_path, capsys):
    """train.py --decoder gpu --cache-gb 1 --num-workers 2 against --decoder pillow on the same pictures (the pixel path reads
    them from .npy arrays beside the files: no Pillow needed)."""
    files = js.ok_files(js.golden())[:32]
    js.write_dataset(tmp_path / 'jpg', files, NUM_VALID)
    js.write_dataset(tmp_path / 'npy', files, NUM_VALID, npy_beside=True)
    common = ['--epochs', '2', '--batch-size', '4', '--data-source', 'jpegset', '--checkpoint-interval', '5', '--lr-values', '0.0001',
              '--lr-boundaries', '', '--tensorboard-dir', str(tmp_path / 'tb')]
    a, b = str(tmp_path / 'pillow'), str(tmp_path / 'gpu')
    assert train.main(['--name', a, '--data-dir', str(tmp_path / 'npy'), '--decoder', 'pillow'] + common) == 0
    out_a = capsys.readouterr().out
    assert train.main(['--name', b, '--data-dir', str(tmp_path / 'jpg'), '--decoder', 'gpu', '--cache-gb', '1', '--num-workers', '2'] + common) == 0
    out_b = capsys.readouterr().out
    assert '[i] Decoder:               gpu' in out_b and '[i] Decoder:               pillow' in out_a
    pick = lambda o: [l for l in o.splitlines() if l.startswith(('[i] Train', '[i] Valid', '[i] mAP'))]
    assert pick(out_a) == pick(out_b) and len(pick(out_a)) == 6
    ca, cb = np.load(a + '/final.npz'), np.load(b + '/final.npz')
    for k in ca.files:
        assert np.array_equal(ca[k], cb[k]), k
    assert train.main(['--name', b, '--data-dir', str(tmp_path / 'jpg'), '--cache-gb', '1'] + common) == 1      # the cache needs --decoder gpu
