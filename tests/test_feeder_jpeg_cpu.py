"""CPU half of the feeder with decoder='gpu' (DESIGN.md 17): what the workers ship when the JPEGs are decoded on the GPU, with the
GPU half of a batch replaced by a host stand-in (as tests/test_feeder_cpu.py does).  The reference of every comparison is the pixel
path: the same TrainingData with images={filename: libjpeg-turbo's pixels} and the default decoder.  The real thing is
tests/test_gpu_feeder_jpeg.py."""
import ctypes as C

import numpy as np
import pytest

import source_jpegset as js
from oracle import boxes as ob
from ssd_tensorflow_amd import jpeg, ssdutils
from ssd_tensorflow_amd import transforms as T
from ssd_tensorflow_amd.parallel import ShardSampler
from ssd_tensorflow_amd.training_data import SRC_CACHED, SRC_COEF, SRC_PIXELS, TrainingData

BATCH = 4


def _prime():
    preset = ssdutils.get_preset_by_name('vgg300')
    ssdutils.prime_anchor_table(preset, ob.anchors_abs(ob.anchors(ob.PRESETS['vgg300'])))


def _host_upload(arrays, gts, slot):
    return {k: np.array(v) for k, v in arrays.items()}, [[tuple(b) for b in g] for g in gts]


def _td(root, **kw):
    _prime()
    td = TrainingData(str(root), 'vgg300', data_source='jpegset', device_tensors=False, **kw)
    td._upload_hook = _host_upload
    return td


def _collect(td, which, workers, epoch):
    td.epoch = epoch
    gen = td.train_generator if which == 'train' else td.valid_generator
    return [(x, y, gt) for x, y, gt in gen(BATCH, workers)]


def _indices(td, which, epoch):
    r = td._recipes[which]
    return [idx for idx, _ in ShardSampler(r.total, BATCH, td.rank, td.world, td.seed + r.salt).batches_with_count(epoch)]


def _params(arrays):
    n = arrays['params'].size // C.sizeof(T._Params)
    return (T._Params * n).from_buffer_copy(arrays['params'].tobytes())


def _params_but_src_off(arrays):
    p = _params(arrays)
    for q in p:
        q.src_off = 0
    return bytes(p)


def _same_decisions(ref, got):
    assert len(ref) == len(got)
    for (xa, ya, ga), (xb, yb, gb) in zip(ref, got):
        assert _params_but_src_off(xa) == _params_but_src_off(xb)
        for k in ('gt', 'gcls', 'goff'):
            assert np.array_equal(xa[k], xb[k]), k
        assert ya == yb and ga == gb


def _disjoint(spans):
    spans = sorted(spans)
    return all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))


@pytest.fixture(scope='module')
def fixture_files():
    return js.ok_files(js.golden())[:28]


@pytest.fixture
def dataset(tmp_path, fixture_files):
    images = js.write_dataset(tmp_path, fixture_files, 8)
    return tmp_path, images


def test_worker_arrays_hold_the_pixel_paths_decisions_and_the_files_coefficients(dataset):
    root, images = dataset
    ref, td = _td(root, images=images), _td(root, decoder='gpu')
    try:
        for which, workers, epoch in (('train', 0, 0), ('train', 2, 0), ('train', 2, 1), ('valid', 0, 0), ('valid', 2, 1)):
            want, got = _collect(ref, which, 0, epoch), _collect(td, which, workers, epoch)
            _same_decisions(want, got)
            samples = td.train_samples if which == 'train' else td.valid_samples
            for idx, (x, _, _) in zip(_indices(td, which, epoch), got):
                p = _params(x)
                assert x['coef'].dtype == np.int16 and x['packed'].size == 0
                assert list(x['src_kind']) == [SRC_COEF] * len(idx)
                descs = (jpeg.Desc * len(idx)).from_buffer_copy(x['descs'].tobytes())
                src, coef = [], []
                for k, i in enumerate(idx):
                    with open(samples[int(i)].filename, 'rb') as f:
                        data = f.read()
                    st, d, c = jpeg.entropy_decode(data)
                    assert st == jpeg.OK
                    n = jpeg.lib.ssd_jpeg_coef_bytes(data, len(data)) // 2
                    base = descs[k].coef_off[0]
                    assert base % 8 == 0                                         # 16 bytes
                    assert np.array_equal(x['coef'][base:base + n], c[:n])
                    for name, _ in jpeg.Desc._fields_:
                        if name == 'coef_off':
                            assert [v - base for v in descs[k].coef_off] == list(d.coef_off)
                        elif name == 'qt':
                            assert bytes(descs[k].qt) == bytes(d.qt)
                        elif name != 'dst_off':
                            assert getattr(descs[k], name) == getattr(d, name), name
                    assert descs[k].dst_off == p[k].src_off and p[k].src_off % 16 == 0
                    assert (p[k].src_h, p[k].src_w) == images[samples[int(i)].filename].shape[:2]
                    src.append((p[k].src_off, p[k].src_off + p[k].src_h * p[k].src_w * 3))
                    coef.append((base, base + n))
                assert _disjoint(src) and _disjoint(coef) and max(e for _, e in coef) <= x['coef'].size
    finally:
        ref.close(); td.close()


def test_a_file_is_read_once_per_sample_whatever_the_redraw_loop_does(dataset, monkeypatch):
    root, _ = dataset
    td = _td(root, decoder='gpu')
    opened, loads = [], []
    real_open, real_call = open, T.ImageLoaderTransform.__call__

    def counting_open(name, *a, **k):
        opened.append(str(name))
        return real_open(name, *a, **k)

    def counting_call(self, data, label, gt):
        loads.append(gt.filename)
        return real_call(self, data, label, gt)

    monkeypatch.setattr(T, 'open', counting_open, raising=False)
    monkeypatch.setattr(T.ImageLoaderTransform, '__call__', counting_call)
    try:
        for epoch in (0, 1):
            del opened[:], loads[:]
            _collect(td, 'train', 0, epoch)
            names = sorted(s.filename for s in td.train_samples)
            assert sorted(opened) == names                       # once each ...
            assert sorted(set(loads)) == names and len(loads) > len(names)      # ... although some samples were drawn again
    finally:
        td.close()


def test_a_file_beyond_the_range_guard_takes_the_pixel_path_with_the_same_decisions(tmp_path, fixture_files, monkeypatch):
    z = js.golden()
    pixels = np.random.default_rng(3).integers(0, 256, (8, 8, 3), dtype=np.uint8)
    files = fixture_files[:6] + [('guard_beyond', z['guard_beyond_jpg'].tobytes(), pixels)] + fixture_files[6:11]
    images = js.write_dataset(tmp_path, files, 0)
    guard = [f for f in images if 'guard_beyond' in f][0]
    real_load = T.load_image_bgr
    monkeypatch.setattr(T, 'load_image_bgr', lambda f: pixels if f == guard else real_load(f))      # (the decode itself: no Pillow needed)
    ref, td = _td(tmp_path, images=images), _td(tmp_path, decoder='gpu')
    try:
        want, got = _collect(ref, 'train', 0, 0), _collect(td, 'train', 0, 0)
        _same_decisions(want, got)
        seen = 0
        for idx, (x, _, _) in zip(_indices(td, 'train', 0), got):
            p = _params(x)
            for k, i in enumerate(idx):
                is_guard = td.train_samples[int(i)].filename == guard
                assert x['src_kind'][k] == (SRC_PIXELS if is_guard else SRC_COEF)
                if is_guard:
                    seen += 1
                    assert np.array_equal(x['packed'][:192], pixels.reshape(-1)) and x['packed'].size == 192
                    assert x['descs'].size == (len(idx) - 1) * C.sizeof(jpeg.Desc)
                    # the pixels lie behind the decoded pictures
                    assert p[k].src_off == sum((q.src_h * q.src_w * 3 + 15) // 16 * 16 for n, q in enumerate(p) if n != k)
        assert seen == 1
    finally:
        ref.close(); td.close()


def test_a_corrupt_file_is_a_jpeg_error_that_names_it_and_the_pool_goes_on(tmp_path, fixture_files):
    z = js.golden()
    files = fixture_files[:5] + [('broken', z['bad_0_jpg'].tobytes(), (80, 96))] + fixture_files[5:10]
    images = js.write_dataset(tmp_path, files, 0)
    broken = str(tmp_path / 'broken.jpg')
    images[broken] = np.zeros((80, 96, 3), np.uint8)
    ref, td = _td(tmp_path, images=images), _td(tmp_path, decoder='gpu')
    try:
        with pytest.raises(RuntimeError, match=r'JpegError: .*broken\.jpg: jpeg: entropy-coded data ends early'):
            _collect(td, 'train', 2, 0)
        pool = td._recipes['train'].pool
        with open(broken, 'wb') as f:                            # the file is repaired: the SAME workers serve the next epoch
            f.write(z['bad_source_jpg'].tobytes())
        got = _collect(td, 'train', 2, 1)
        assert td._recipes['train'].pool is pool and len(got) == 3
        _same_decisions(_collect(ref, 'train', 0, 1), got)
        # a corrupt HEADER is refused by the loader, in whichever process plans the sample
        with open(broken, 'wb') as f:
            f.write(z['bad_3_jpg'].tobytes())
        with pytest.raises(jpeg.JpegError, match=r'broken\.jpg: jpeg: Huffman table counts'):
            _collect(td, 'train', 0, 0)
    finally:
        ref.close(); td.close()


def test_a_cached_samples_task_opens_no_file(dataset, monkeypatch):
    root, images = dataset
    td = _td(root, decoder='gpu')
    try:
        idx = _indices(td, 'train', 0)[1]
        recipe = td._recipes['train']
        want, want_gts = recipe.plan(0, idx)
        opened = []
        real_open = open
        monkeypatch.setattr(T, 'open', lambda name, *a, **k: opened.append(name) or real_open(name, *a, **k), raising=False)
        known = {k: images[td.train_samples[int(i)].filename].shape[:2] for k, i in enumerate(idx)}
        got, gts = recipe.plan(0, idx, known)
        assert opened == [] and gts == want_gts
        assert list(got['src_kind']) == [SRC_CACHED] * len(idx)
        assert got['coef'].size == got['packed'].size == got['descs'].size == 0
        assert _params_but_src_off(got) == _params_but_src_off(want)
        # a batch of which only some samples are cached: the others are read and ship coefficients
        del known[1]
        got, _ = recipe.plan(0, idx, known)
        assert opened == [td.train_samples[int(idx[1])].filename]
        assert list(got['src_kind']) == [SRC_CACHED, SRC_COEF] + [SRC_CACHED] * (len(idx) - 2)
        assert got['descs'].size == C.sizeof(jpeg.Desc) and _params_but_src_off(got) == _params_but_src_off(want)
    finally:
        td.close()


def test_the_arguments_are_checked(dataset):
    root, _ = dataset
    with pytest.raises(ValueError, match='decoder'):
        TrainingData(str(root), 'vgg300', data_source='jpegset', decoder='opencv')
    with pytest.raises(ValueError, match='cache_bytes'):
        TrainingData(str(root), 'vgg300', data_source='jpegset', cache_bytes=1 << 20)
    with pytest.raises(ValueError, match='cache_bytes'):
        TrainingData(None, 'vgg300', cache_bytes=1 << 20, decoder='pillow')
    with pytest.raises(ValueError, match='decoder'):
        T.build_valid_transforms(ssdutils.get_preset_by_name('vgg300'), 20, decoder='cv2')
    # the synthetic sets hold arrays: decoder='gpu' changes nothing about what their workers ship
    _prime()
    a = TrainingData(None, 'vgg300', num_train=8, num_valid=4, augment=True, device_tensors=False)
    b = TrainingData(None, 'vgg300', num_train=8, num_valid=4, augment=True, device_tensors=False, decoder='gpu')
    a._upload_hook = b._upload_hook = _host_upload
    try:
        for (xa, ya, ga), (xb, yb, gb) in zip(a.train_generator(4, 0), b.train_generator(4, 0)):
            assert xa.keys() == xb.keys() and all(np.array_equal(xa[k], xb[k]) for k in xa) and ga == gb
    finally:
        a.close(); b.close()
