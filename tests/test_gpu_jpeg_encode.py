"""GPU: the JPEG encode kernel (csrc/jpeg_enc.hip) against the numpy oracle tests/jpeg_enc_ref.py, which
tests/test_jpeg_encode.py pins against libjpeg-turbo's own files (tests/golden/j2_jpeg_encode.npz); jpeg.encode_batch end to end;
the drivers' --encoder gpu.  Reads only files of this repository.  Everything is exact: no tolerance, no case left out.  Nothing
here sends bad arguments to a kernel: the device entry point refuses them before it launches."""
import ctypes as C
import filecmp
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import jpeg_enc_ref
import jpeg_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'j2_jpeg_encode.npz')
QUALITIES = [1, 30, 75, 95, 100]
SAMPLINGS = ['4:4:4', '4:2:2', '4:2:0']


@pytest.fixture(scope='module')
def g():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope='module')
def oracle(g):
    """{(picture index, quality, sampling): (Desc, coefficients)} of every fixture case"""
    return {(int(g['case_src'][i]), int(g['case_quality'][i]), str(g['case_sampling'][i])):
            jpeg_enc_ref.encode_planes(g['src_%d_bgr' % g['case_src'][i]], int(g['case_quality'][i]), str(g['case_sampling'][i]))
            for i in range(len(g['case_names']))}


def pictures(g):
    return [g['src_%d_bgr' % j] for j in range(len(g['src_names']))]


def pillow_file(g, j, q, s):
    i = next(i for i in range(len(g['case_names'])) if (int(g['case_src'][i]), int(g['case_quality'][i]), str(g['case_sampling'][i])) == (j, q, s))
    return g['case_%d_jpg' % i].tobytes()


def device_stage(images, quality, subsampling, gap=0):
    """ssd_jpeg_encode_batch_dev on a packed upload of `images` -> (int16 coefficients on the host, Desc array)"""
    import torch
    from ssd_tensorflow_amd import jpeg, _lib
    n = len(images)
    offs, total = [], gap
    for a in images:
        offs.append(total)
        total += (a.size + 15) // 16 * 16 + gap
    host = np.zeros(total, np.uint8)
    for a, o in zip(images, offs):
        host[o:o + a.size] = a.reshape(-1)
    dev = torch.device('cuda', 0)
    src = torch.from_numpy(host).to(dev)
    shp = (C.c_int * (2 * n))(*[int(v) for a in images for v in a.shape[:2]])
    src_offs = (C.c_ulonglong * n)(*offs)
    sampling = jpeg.SAMPLING[subsampling]
    coef_bytes, ws_bytes = _lib.lib.ssd_jpeg_enc_coef_bytes(shp, n, sampling), _lib.lib.ssd_jpeg_enc_ws_bytes(shp, n, sampling)
    assert coef_bytes > 0 and ws_bytes > 0, _lib.last_error()
    coef = torch.full((coef_bytes // 2,), 0x5a5a, dtype=torch.int16, device=dev)          # (every coefficient must be written)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    descs = (jpeg.Desc * n)()
    rc = _lib.lib.ssd_jpeg_encode_batch_dev(src.data_ptr(), src.numel(), src_offs, shp, n, quality, sampling, coef.data_ptr(), coef_bytes,
                                            descs, ws.data_ptr(), ws_bytes, torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    return coef.cpu().numpy(), descs


def check_image(name, coef, d, want, base=None):
    """descriptor d of a batch's coefficient buffer against the oracle's (e, coefficients)"""
    e, wc = want
    assert (d.width, d.height, d.components, d.hs, d.vs, d.mcus_x, d.mcus_y) == (e.width, e.height, 3, e.hs, e.vs, e.mcus_x, e.mcus_y), name
    assert [list(t) for t in d.qt] == e.qt, name
    base = int(d.coef_off[0]) if base is None else base
    assert [int(d.coef_off[c]) - base for c in range(3)] == e.coef_off, name
    got = coef[base:base + wc.size]
    assert np.array_equal(got, wc), '%s: %d coefficients differ, first at %s' % (name, int((got != wc).sum()), np.nonzero(got != wc)[0][:4])
    return base + wc.size


@pytest.mark.parametrize('subsampling', SAMPLINGS)
def test_device_coefficients_one_mixed_batch(g, oracle, subsampling):
    """every fixture picture, all sizes in one launch per quality: coefficients and descriptors equal the oracle's exactly"""
    pics = pictures(g)
    for q in QUALITIES:
        coef, descs = device_stage(pics, q, subsampling, gap=(q % 3) * 5)       # (sources at unaligned offsets as well)
        end = 0
        for j in range(len(pics)):
            assert int(descs[j].coef_off[0]) == end                              # one image after the other, nothing between them
            end = check_image('%s q%d %s' % (g['src_names'][j], q, subsampling), coef, descs[j], oracle[(j, q, subsampling)])
        assert end == coef.size


def test_device_coefficients_one_by_one(g, oracle):
    pics = pictures(g)
    for (j, q, s), want in sorted(oracle.items()):
        coef, descs = device_stage([pics[j]], q, s)
        assert check_image('%s q%d %s' % (g['src_names'][j], q, s), coef, descs[0], want, base=0) == coef.size


def _ctypes_desc(e):
    from ssd_tensorflow_amd import jpeg
    d = jpeg.Desc()
    d.width, d.height, d.components, d.hs, d.vs, d.mcus_x, d.mcus_y = e.width, e.height, 3, e.hs, e.vs, e.mcus_x, e.mcus_y
    for c in range(3):
        d.coef_off[c] = e.coef_off[c]
        for k in range(64):
            d.qt[c][k] = e.qt[c][k]
    return d


def test_files_equal_the_host_stage_on_the_oracle_and_libjpeg(g, oracle):
    """jpeg.encode_batch == the host stage on the oracle's coefficients == the file Pillow wrote, byte for byte"""
    from ssd_tensorflow_amd import jpeg
    pics = pictures(g)
    for s in SAMPLINGS:
        for q in QUALITIES:
            files = jpeg.encode_batch(pics, quality=q, subsampling=s)
            assert len(files) == len(pics)
            for j, data in enumerate(files):
                e, wc = oracle[(j, q, s)]
                assert data == jpeg.entropy_encode(wc, _ctypes_desc(e)), (str(g['src_names'][j]), q, s)
                assert data == pillow_file(g, j, q, s), (str(g['src_names'][j]), q, s)
    assert jpeg.encode(pics[5]) == pillow_file(g, 5, 95, '4:2:0')               # the defaults are cv2.imwrite's
    assert jpeg.encode_batch(pics[:3], threads=1) == [pillow_file(g, j, 95, '4:2:0') for j in range(3)]


def test_device_tensor_source_and_repeatability(g):
    """a device tensor with offsets (what annotate_batch leaves) gives the files of the host arrays; two launches, identical bytes"""
    import torch
    from ssd_tensorflow_amd import jpeg, annotate
    pics = pictures(g)
    shapes = [p.shape[:2] for p in pics]
    offs, total = annotate.pack_offsets(shapes, 1)
    host = np.zeros(total, np.uint8)
    for p, o in zip(pics, offs):
        host[o:o + p.size] = p.reshape(-1)
    src = torch.from_numpy(host).cuda()
    a = jpeg.encode_batch(src, offs, shapes, quality=75, subsampling='4:2:2', threads=3)
    b = jpeg.encode_batch(src, offs, shapes, quality=75, subsampling='4:2:2', threads=8)
    assert a == b == [pillow_file(g, j, 75, '4:2:2') for j in range(len(pics))]
    picks = [7, 2, 20]                                                          # a subset, out of order
    assert jpeg.encode_batch(src, [offs[j] for j in picks], [shapes[j] for j in picks], quality=75, subsampling='4:2:2') == [a[j] for j in picks]
    c1, _ = device_stage(pics, 95, '4:2:0')
    c2, _ = device_stage(pics, 95, '4:2:0')
    assert np.array_equal(c1, c2)
    s = torch.cuda.Stream()
    t1 = jpeg.encode_launch(src, offs, shapes, stream=s)
    t2 = jpeg.encode_launch(pics, stream=s)
    assert t1.get() == t2.get() == [pillow_file(g, j, 95, '4:2:0') for j in range(len(pics))]


def test_round_trip_through_the_decoder(g, oracle):
    """decode_batch(encode_batch(x)) == the reference back half applied to the oracle's coefficients"""
    from ssd_tensorflow_amd import jpeg
    pics = pictures(g)
    for s in SAMPLINGS:
        for q in QUALITIES:
            dst, offs, sizes, fallbacks = jpeg.decode_batch(jpeg.encode_batch(pics, quality=q, subsampling=s))
            assert fallbacks == []
            host = dst.cpu().numpy()
            for j, p in enumerate(pics):
                e, wc = oracle[(j, q, s)]
                want = jpeg_ref.decode_planes(wc, e)
                assert sizes[j] == p.shape[:2] and np.array_equal(host[offs[j]:offs[j] + p.size].reshape(p.shape), want), (str(g['src_names'][j]), q, s)


def test_extremes():
    """constant 0, constant 255, a 0 / 255 checkerboard at quality 100 (the largest coefficient of the highest frequency), strips of
    16384 x 1 and 1 x 16384"""
    from ssd_tensorflow_amd import jpeg
    y, x = np.mgrid[0:40, 0:56]
    board = np.repeat((((x + y) & 1) * 255).astype(np.uint8)[:, :, None], 3, 2)
    rng = np.random.default_rng(5)
    imgs = [np.zeros((33, 47, 3), np.uint8), np.full((33, 47, 3), 255, np.uint8), board, np.ascontiguousarray(board[:, :, :] * np.array([1, 0, 1], np.uint8)),
            rng.integers(0, 256, (1, 16384, 3)).astype(np.uint8), rng.integers(0, 256, (16384, 1, 3)).astype(np.uint8)]
    for s in SAMPLINGS:
        for q in (100, 1):
            coef, descs = device_stage(imgs, q, s)
            for k, im in enumerate(imgs):
                check_image('extreme %d q%d %s' % (k, q, s), coef, descs[k], jpeg_enc_ref.encode_planes(im, q, s))
    e, wc = jpeg_enc_ref.encode_planes(board, 100, '4:4:4')
    assert abs(int(wc[63])) >= 800                                             # the checkerboard does reach the corner coefficient
    files = jpeg.encode_batch(imgs, quality=100, subsampling='4:4:4')
    for im, data in zip(imgs, files):
        e, wc = jpeg_enc_ref.encode_planes(im, 100, '4:4:4')
        assert data == jpeg.entropy_encode(wc, _ctypes_desc(e))
        st, d, coef = jpeg.entropy_decode(data)
        assert st in (jpeg.OK, jpeg.UNSUPPORTED) and (d.width, d.height) == (im.shape[1], im.shape[0])


def test_device_entry_point_refuses_before_it_launches(g):
    """every refused call below would stay inside the real buffers if it were launched: the declared sizes are what is wrong"""
    import torch
    from ssd_tensorflow_amd import jpeg, _lib
    pics = pictures(g)[8:11]
    n = 3
    offs, total = [], 0
    for a in pics:
        offs.append(total)
        total += (a.size + 15) // 16 * 16
    host = np.zeros(total + 64, np.uint8)
    for a, o in zip(pics, offs):
        host[o:o + a.size] = a.reshape(-1)
    dev = torch.device('cuda', 0)
    src = torch.from_numpy(host).to(dev)
    shapes = [list(a.shape[:2]) for a in pics]
    s = torch.cuda.current_stream(dev).cuda_stream

    def sizes(shapes=shapes, n=n, sampling=0x22):
        shp = (C.c_int * (2 * len(shapes)))(*[v for hw in shapes for v in hw])
        return _lib.lib.ssd_jpeg_enc_coef_bytes(shp, n, sampling), _lib.lib.ssd_jpeg_enc_ws_bytes(shp, n, sampling)

    coef_bytes, ws_bytes = sizes()
    assert coef_bytes > 0 and ws_bytes > 0
    coef = torch.zeros((coef_bytes // 2 + 64,), dtype=torch.int16, device=dev)
    ws = torch.empty((ws_bytes + 256,), dtype=torch.uint8, device=dev)
    descs = (jpeg.Desc * n)()

    def run(shapes=shapes, offs=offs, n=n, quality=95, sampling=0x22, src_bytes=total, coef_b=coef_bytes, ws_b=ws_bytes, coef_ptr=None, ws_ptr=None):
        shp = (C.c_int * (2 * len(shapes)))(*[v for hw in shapes for v in hw])
        so = (C.c_ulonglong * len(offs))(*offs)
        return _lib.lib.ssd_jpeg_encode_batch_dev(src.data_ptr(), src_bytes, so, shp, n, quality, sampling, coef_ptr or coef.data_ptr(), coef_b,
                                                  descs, ws_ptr or ws.data_ptr(), ws_b, s)

    assert run() == 0, _lib.last_error()
    torch.cuda.synchronize()
    good = coef.cpu().numpy().copy()
    assert good.any()
    h1, w1 = shapes[1]
    for kw, text in ((dict(quality=0), 'quality'), (dict(quality=101), 'quality'), (dict(sampling=0x12), 'sampling'), (dict(sampling=0x41), 'sampling'),
                     (dict(sampling=0), 'sampling'), (dict(n=0), 'empty batch'), (dict(src_bytes=total - 16), 'source'),
                     (dict(src_bytes=offs[2] + pics[2].size - 1), 'source'), (dict(offs=[offs[0], total, offs[2]]), 'source'),
                     (dict(coef_b=coef_bytes - 128), 'coefficient buffer'), (dict(ws_b=ws_bytes - 256), 'workspace'),
                     (dict(shapes=[shapes[0], [0, w1], shapes[2]]), 'size'), (dict(shapes=[shapes[0], [h1, 16385], shapes[2]]), 'size'),
                     (dict(coef_ptr=coef.data_ptr() + 2), 'aligned'), (dict(ws_ptr=ws.data_ptr() + 8), 'aligned')):
        assert run(**kw) != 0, kw
        assert re.search(text, _lib.last_error()), (kw, _lib.last_error())
    assert sizes(sampling=0x12) == (0, 0) and sizes(n=0) == (0, 0) and sizes(shapes=[shapes[0], [0, 5], shapes[2]]) == (0, 0)
    for bad in (dict(quality=0), dict(subsampling='4:1:1')):
        with pytest.raises((jpeg.JpegError, ValueError)):
            jpeg.encode_batch(pics, **bad)
    torch.cuda.synchronize()
    assert np.array_equal(coef.cpu().numpy(), good)                    # the refused calls wrote nothing
    assert run() == 0


def _child(args, seconds=600):
    r = subprocess.run([sys.executable, '-m'] + args, cwd=ROOT, capture_output=True, text=True, timeout=seconds)
    assert r.returncode == 0, '%s\n%s\n%s' % (args, r.stdout[-1500:], r.stderr[-3000:])
    return r.stdout


def test_drivers_with_the_gpu_encoder(g, tmp_path):
    """detect.py --encoder gpu and --encoder pillow on five generated JPEGs and one .npy array, as child processes: every .jpg the
    gpu encoder wrote equals jpeg.encode_batch of the pixels --encoder pillow draws (fetched here through
    annotate_last_launch(...).get() on the same model and batches), the .txt files do not change, the array's picture still goes
    through write_image; infer.py --annotate --encoder gpu writes JPEGs of the right sizes and counts the same detections."""
    pytest.importorskip('PIL.Image')
    import torch
    from ssd_tensorflow_amd import jpeg
    from ssd_tensorflow_amd.annotate import Style
    from ssd_tensorflow_amd.infer import sample_generator, resolve_class_names
    from ssd_tensorflow_amd.ssdvgg import SSDVGG, Session
    from ssd_tensorflow_amd.ssdutils import get_preset_by_name
    from ssd_tensorflow_amd.utils import default_colors
    names = [str(n) for n in g['src_names']]
    picks = [j for j, n in enumerate(names) if n.endswith(('144x96', '104x88', '81x80', '95x65', '47x63'))][:5]
    assert len(picks) == 5
    files = []
    for k, j in enumerate(picks):
        files.append(str(tmp_path / (names[j] + ('.jpeg' if k == 1 else '.jpg'))))
        open(files[-1], 'wb').write(pillow_file(g, j, 95, '4:4:4'))
    arr = str(tmp_path / 'array.npy')
    np.save(arr, g['src_%d_bgr' % picks[0]])
    files.insert(2, arr)
    model = str(tmp_path / 'model.npz')
    with Session(0) as sess:
        net = SSDVGG(sess, 'vgg300')
        net.build_from_vgg(None, 3, max_batch=4)
        net.build_optimizer()
        net.save_checkpoint(model, class_names=['class_%d' % i for i in range(3)])
    out = {}
    for enc in ('gpu', 'pillow'):
        out[enc] = str(tmp_path / ('detect_' + enc))
        _child(['ssd_tensorflow_amd.detect', '--model', model, '--output-dir', out[enc], '--batch-size', '4', '--encoder', enc] + files)
    listing = sorted(os.listdir(out['gpu']))
    assert listing == sorted(os.listdir(out['pillow'])) and len(listing) == 12, listing
    txt = [n for n in listing if n.endswith('.txt')]
    assert len(txt) == 6
    match, mismatch, errors = filecmp.cmpfiles(out['gpu'], out['pillow'], txt + ['array.npy.png'], shallow=False)
    assert not mismatch and not errors, (mismatch, errors)
    # the pixels --encoder pillow draws, on the same model and the same batches
    drawn = {}
    with Session(0) as sess:
        with np.load(model, allow_pickle=False) as ck:
            stored = ck['__class_names__']
        net = SSDVGG(sess, get_preset_by_name('vgg300'))
        net.build_from_metagraph(None, model, max_batch=4, dtype='f32')
        lid2name = resolve_class_names(3, None, stored)
        cnames = [str(lid2name[i]) for i in range(3)]
        colors = default_colors(cnames)
        style = Style([colors[n] for n in cnames], cnames, sess.device)
        for x, idxs, sizes, sources in sample_generator(files, net.preset.image_size, 4, with_sources=True, decoder='gpu'):
            net.infer_dev(x)
            net.detect_last_launch(x.shape[0], 0.5, None, 200)
            for i, img in zip(idxs, net.annotate_last_launch(*sources, style).get()):
                drawn[os.path.basename(files[i])] = img.copy()
        style.close()
    jpgs = [n for n in listing if n.endswith(('.jpg', '.jpeg'))]
    assert len(jpgs) == 5
    want = jpeg.encode_batch([drawn[n] for n in jpgs])
    for n, data in zip(jpgs, want):
        assert open(os.path.join(out['gpu'], n), 'rb').read() == data, n
        assert open(os.path.join(out['pillow'], n), 'rb').read() != data, n          # (Pillow's own default is quality 75)
    q50 = str(tmp_path / 'detect_q50')
    _child(['ssd_tensorflow_amd.detect', '--model', model, '--output-dir', q50, '--batch-size', '4', '--encoder', 'gpu', '--jpeg-quality', '50'] + files[:2])
    first = os.path.basename(files[0])
    assert open(os.path.join(q50, first), 'rb').read() == jpeg.encode_batch([drawn[first]], quality=50)[0]
    lines = {}
    for enc in ('gpu', 'pillow'):
        out[enc] = str(tmp_path / ('infer_' + enc))
        text = _child(['ssd_tensorflow_amd.infer', '--preset', 'vgg300', '--name', str(tmp_path / 'none'), '--threshold', '0.05',
                       '--batch-size', '4', '--annotate', 'true', '--output-dir', out[enc], '--encoder', enc] + files)
        lines[enc] = [l for l in text.splitlines() if l.startswith('[i] Processed')]
    assert lines['gpu'] == lines['pillow'] and lines['gpu'][0].startswith('[i] Processed 6 images') and not lines['gpu'][0].endswith(' 0 detections')
    assert sorted(os.listdir(out['gpu'])) == sorted(os.listdir(out['pillow']))
    for n in jpgs:
        data = open(os.path.join(out['gpu'], n), 'rb').read()
        w, h, comps, sampling, st = jpeg.info(data)
        assert (h, w) == drawn[n].shape[:2] and (comps, sampling, st) == (3, 0x22, jpeg.OK), n
        assert jpeg.entropy_decode(data)[0] == jpeg.OK
