"""GPU: the JPEG decode kernels (csrc/jpeg.hip) against the pixels libjpeg-turbo produces
(tests/golden/j1_jpeg.npz), device-resident sources in augment_batch, and the drivers' --decoder gpu.  Reads only files of this
repository.  Nothing here sends bad data to a kernel: corrupt files stop in the host stage (tests/test_jpeg.py) and the device
entry point refuses inconsistent descriptors before it launches."""
import filecmp
import hashlib
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import jpeg_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'j1_jpeg.npz')


@pytest.fixture(scope='module')
def g():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _ok(g):
    return [(str(n), g['ok_%d_jpg' % i].tobytes(), g['ok_%d_bgr' % i]) for i, n in enumerate(g['ok_names'])]


def test_decode_equals_libjpeg_file_by_file(g):
    """6, first half (and 7: no file may fall back)"""
    from ssd_tensorflow_amd import jpeg
    ok = _ok(g)
    assert len(ok) >= 40
    for name, data, want in ok:
        dst, offs, sizes, fallbacks = jpeg.decode_batch([data], threads=1)
        assert fallbacks == [] and sizes == [want.shape[:2]], name
        got = dst[:want.size].cpu().numpy().reshape(want.shape)
        assert np.array_equal(got, want), '%s: %d bytes differ' % (name, int((got != want).sum()))
        assert np.array_equal(jpeg.decode(data), want), name


@pytest.mark.parametrize('threads', [None, 1, 5])
def test_decode_one_batch_of_everything(g, threads):
    """6, second half: all supported files and the two VOC pictures in one batch, one launch pair"""
    from ssd_tensorflow_amd import jpeg
    ok = _ok(g)
    voc = [str(n) for n in g['voc_names']]
    datas = [d for _, d, _ in ok] + [g['voc_%s_jpg' % n].tobytes() for n in voc]
    dst, offs, sizes, fallbacks = jpeg.decode_batch(datas, threads=threads)
    assert fallbacks == []
    host = dst.cpu().numpy()
    end = 0
    for i, (name, _, want) in enumerate(ok):
        assert offs[i] % 16 == 0 and offs[i] >= end and sizes[i] == want.shape[:2]
        end = offs[i] + want.size
        assert np.array_equal(host[offs[i]:end].reshape(want.shape), want), name
    for k, name in enumerate(voc):
        i = len(ok) + k
        h, w = sizes[i]
        assert (h, w) == tuple(g['voc_%s_shape' % name])
        got = host[offs[i]:offs[i] + h * w * 3].reshape(h, w, 3)
        wrong = np.nonzero((got.astype(np.int64).sum(1) != g['voc_%s_rowsums' % name]).any(1))[0]
        assert wrong.size == 0, '%s: rows %s differ' % (name, wrong[:8])
        assert hashlib.sha256(got.tobytes()).hexdigest() == str(g['voc_%s_sha256' % name])


def test_range_guard(g):
    """8: a block whose L1 norm sits exactly on the guard decodes equal to the int64 reference; one past it never reaches a kernel"""
    from ssd_tensorflow_amd import jpeg
    inside, beyond = g['guard_inside_jpg'].tobytes(), g['guard_beyond_jpg'].tobytes()
    st, d, coef = jpeg.entropy_decode(inside)
    assert st == jpeg.OK and d.max_l1 == jpeg.MAX_L1
    want = jpeg_ref.decode_planes(coef, d)
    assert want.min() == 0 and want.max() == 255                       # the block saturates both ways
    dst, offs, sizes, fallbacks = jpeg.decode_batch([inside], threads=1)
    assert fallbacks == [] and np.array_equal(dst[:192].cpu().numpy().reshape(8, 8, 3), want)
    assert jpeg.entropy_decode(beyond)[0] == jpeg.UNSUPPORTED
    pytest.importorskip('PIL.Image')                                   # (the fallback of a bytes item is Pillow)
    dst, offs, sizes, fallbacks = jpeg.decode_batch([inside, beyond], threads=2)
    assert fallbacks == [1] and sizes == [(8, 8), (8, 8)]


def test_device_entry_point_refuses_inconsistent_descriptors(g):
    """every refused call below would stay inside the real buffers if it were launched: the declared sizes are what is wrong"""
    import torch
    from ssd_tensorflow_amd import jpeg, _lib
    datas = [g['ok_%d_jpg' % i] for i in (0, 1, 2)]
    coef, offs, descs, status, _ = jpeg.entropy_decode_batch(datas, threads=1)
    assert status == [jpeg.OK] * 3
    off = 0
    for d in descs:
        d.dst_off = off
        off += (d.width * d.height * 3 + 15) // 16 * 16
    dev = torch.device('cuda', 0)
    coef_dev = torch.from_numpy(coef).to(dev)
    dst = torch.zeros((off + 64,), dtype=torch.uint8, device=dev)
    ws_bytes = _lib.lib.ssd_jpeg_ws_bytes(descs, 3)
    assert ws_bytes > 0
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream

    def run(coef_bytes=coef.nbytes, dst_bytes=off, ws_b=ws_bytes, n=3):
        return _lib.lib.ssd_jpeg_decode_batch_dev(coef_dev.data_ptr(), coef_bytes, descs, n, dst.data_ptr(), dst_bytes, ws.data_ptr(), ws_b, s)

    assert run() == 0
    torch.cuda.synchronize()
    good = dst.cpu().numpy().copy()
    for kw, text in ((dict(coef_bytes=coef.nbytes - 128), 'coefficient plane'), (dict(dst_bytes=off - 16), 'destination'),
                     (dict(ws_b=ws_bytes - 256), 'workspace'), (dict(n=0), 'empty batch')):
        assert run(**kw) != 0 and text in _lib.last_error(), kw
    for field, value, text in (('dst_off', 8, 'destination'), ('max_l1', jpeg.MAX_L1 + 1, 'range guard'), ('mcus_x', 0, 'MCUs'),
                               ('hs', 3, 'sampling'), ('width', 0, 'size')):
        keep = getattr(descs[1], field)
        setattr(descs[1], field, descs[1].dst_off + value if field == 'dst_off' else value)
        assert run() != 0 and text in _lib.last_error(), field
        assert _lib.lib.ssd_jpeg_ws_bytes(descs, 3) == (ws_bytes if field in ('dst_off', 'max_l1') else 0)
        setattr(descs[1], field, keep)
    torch.cuda.synchronize()
    assert np.array_equal(dst.cpu().numpy(), good)                    # the refused calls wrote nothing
    assert run() == 0


def _box_sample(size):
    from ssd_tensorflow_amd.utils import Sample, Box, Point, Size
    return Sample('im', [Box('c1', 1, Point(0.5, 0.5), Size(0.5, 0.6)), Box('c2', 2, Point(0.3, 0.4), Size(0.2, 0.3))], Size(*size))


def test_augment_batch_on_device_sources(g):
    """9: plans that read the decoded buffer where it lies == the same plans on host arrays of the same pixels, bit for bit"""
    import torch
    from ssd_tensorflow_amd import jpeg, transforms as T
    from ssd_tensorflow_amd.ssdutils import get_preset_by_name
    names = [str(n) for n in g['ok_names']]
    picks = [names.index(n) for n in names if n.endswith(('104x88', '144x96', '80x81', '95x65'))][:5]
    assert len(picks) == 5
    datas = [g['ok_%d_jpg' % i].tobytes() for i in picks]
    pixels = [g['ok_%d_bgr' % i] for i in picks]
    buf, offs, sizes, fallbacks = jpeg.decode_batch(datas)
    assert fallbacks == []
    preset = get_preset_by_name('vgg300')
    host = []
    plan = T.ImagePlan(pixels[0])
    plan.resize = (300, 300, T.INTER_LINEAR)                           # resize only: the inference path
    host.append(plan)
    for k in range(1, 5):                                              # four plans of the train recipe
        img = pixels[k]
        tfs = [t for t in T.build_train_transforms(preset, 20, 50, 0.5, images={'im': img}) if not isinstance(t, T.LabelCreatorTransform)]
        random.seed(9100 + k)
        args = (None, None, _box_sample((img.shape[1], img.shape[0])))
        for t in tfs:
            args = t(*args)
        host.append(args[0])
    device = []
    for k, p in enumerate(host):
        q = T._copy_plan(p)
        q.image, q.device_src = None, (buf, offs[k])
        device.append(q)
    fresh = T.ImagePlan((buf, offs[0], sizes[0]))
    assert (fresh.src.w, fresh.src.h) == (pixels[0].shape[1], pixels[0].shape[0]) and fresh.shape == pixels[0].shape
    want = T.augment_batch(host, 300, 300)
    got, images, src_offs = T.augment_batch(device, 300, 300, return_images=True)
    assert images is buf and src_offs == offs
    assert torch.equal(got, want)
    arr, packed = T.plan_params(device, 300, 300)
    assert packed is None
    with pytest.raises(ValueError, match='ONE device buffer'):
        T.plan_params([host[0], device[0]], 300, 300)
    with pytest.raises(ValueError, match='does not fit'):
        T.ImagePlan((buf, buf.numel() - 8, (8, 8)))


def _child(args, seconds=600):
    r = subprocess.run([sys.executable, '-m'] + args, cwd=ROOT, capture_output=True, text=True, timeout=seconds)
    assert r.returncode == 0, '%s\n%s\n%s' % (args, r.stdout[-1500:], r.stderr[-3000:])
    return r.stdout


def _same_dirs(a, b, count):
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and len(names) == count, (names, sorted(os.listdir(b)))
    match, mismatch, errors = filecmp.cmpfiles(a, b, names, shallow=False)
    assert not mismatch and not errors, (mismatch, errors)


def test_drivers_with_both_decoders(g, tmp_path):
    """10: detect.py and infer.py --annotate on the same six JPEG files, --decoder gpu and --decoder pillow, as child processes:
    identical detections and identical annotated pictures; a batch that mixes a baseline file, a progressive one and a .npy
    array runs under --decoder gpu."""
    pytest.importorskip('PIL.Image')
    from ssd_tensorflow_amd.ssdvgg import SSDVGG, Session
    names = [str(n) for n in g['ok_names']]
    picks = [n for n in names if n.endswith(('104x88', '144x96', '80x81', '95x65', '47x63'))][:4]
    files = []
    for n in picks:
        files.append(str(tmp_path / (n + '.jpg')))
        open(files[-1], 'wb').write(g['ok_%d_jpg' % names.index(n)].tobytes())
    for n in g['voc_names']:
        files.append(str(tmp_path / (str(n) + '.jpg')))
        open(files[-1], 'wb').write(g['voc_%s_jpg' % n].tobytes())
    assert len(files) == 6
    model = str(tmp_path / 'model.npz')
    with Session(0) as sess:
        net = SSDVGG(sess, 'vgg300')
        net.build_from_vgg(None, 3, max_batch=4)
        net.build_optimizer()
        net.save_checkpoint(model, class_names=['class_%d' % i for i in range(3)])
    out = {}
    for dec in ('gpu', 'pillow'):
        out[dec] = str(tmp_path / ('detect_' + dec))
        _child(['ssd_tensorflow_amd.detect', '--model', model, '--output-dir', out[dec], '--batch-size', '4', '--decoder', dec] + files)
    _same_dirs(out['gpu'], out['pillow'], 12)
    for dec in ('gpu', 'pillow'):
        out[dec] = str(tmp_path / ('infer_' + dec))
        text = _child(['ssd_tensorflow_amd.infer', '--preset', 'vgg300', '--name', str(tmp_path / 'none'), '--threshold', '0.05',
                       '--batch-size', '4', '--annotate', 'true', '--output-dir', out[dec], '--decoder', dec] + files)
        out[dec + '_line'] = [l for l in text.splitlines() if l.startswith('[i] Processed')]
    _same_dirs(out['gpu'], out['pillow'], 6)
    assert out['gpu_line'] == out['pillow_line'] and out['gpu_line'][0].startswith('[i] Processed 6 images')
    assert not out['gpu_line'][0].endswith(' 0 detections')
    # mixed batch: baseline JPEG, progressive JPEG (decoded by the fallback), uint8 .npy array
    prog = str(tmp_path / 'progressive.jpg')
    open(prog, 'wb').write(g['unsup_0_jpg'].tobytes())
    arr = str(tmp_path / 'array.npy')
    np.save(arr, g['ok_%d_bgr' % names.index(picks[1])])
    mixed = [files[0], prog, arr]
    for dec in ('gpu', 'pillow'):
        out[dec] = str(tmp_path / ('mixed_' + dec))
        _child(['ssd_tensorflow_amd.detect', '--model', model, '--output-dir', out[dec], '--batch-size', '4', '--decoder', dec] + mixed)
    _same_dirs(out['gpu'], out['pillow'], 6)
