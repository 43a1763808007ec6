"""GPU: the drivers that draw -- infer.py --annotate, detect.py, train.py's image summaries -- end to end; the pictures they write
are compared with the numpy yardstick (tests/annotate_ref.py) drawn from the same run's detections, for exact equality."""
import os

import numpy as np
import pytest

import annotate_ref as R
from test_annotate import _decode_png
from ssd_tensorflow_amd import infer, detect, train
from ssd_tensorflow_amd import utils as ut
from ssd_tensorflow_amd.ssdutils import boxes_from_detection

pytestmark = pytest.mark.gpu



def _files(tmp_path, sizes, seed=4):
    rng = np.random.default_rng(seed)
    out = []
    for k, (h, w) in enumerate(sizes):
        p = str(tmp_path / ('img%d.npy' % k))
        np.save(p, rng.integers(0, 256, (h, w, 3)).astype(np.uint8))
        out.append(p)
    return out


def _detections(preset, num_classes, files, threshold, ckpt=None):
    """the detections of the same files through the library, the way the drivers obtain them"""
    from ssd_tensorflow_amd.ssdvgg import SSDVGG, Session
    from ssd_tensorflow_amd.ssdutils import get_preset_by_name
    dets = []
    with Session(0) as sess:
        net = SSDVGG(sess, get_preset_by_name(preset))
        if ckpt:
            net.build_from_metagraph(None, ckpt, max_batch=4)
        else:
            net.build_from_vgg(None, num_classes, max_batch=4, training=False)
        for x, idxs, sizes in infer.sample_generator(files, net.preset.image_size, 4):
            net.infer_dev(x)
            dets += [{k: v.copy() for k, v in d.items()} for d in net.detect_last_launch(x.shape[0], threshold, None, 200).get()]
    return dets


def _expected(path, det, names, colors):
    img = np.load(path)
    h, w = img.shape[:2]
    px = [R.rect1000(b, w, h) for b in det['box']]
    return R.draw(img, R.style_boxes(px, det['cls'], colors, names))


def test_infer_annotate(tmp_path, capsys):
    files = _files(tmp_path, [(211, 317), (375, 500)])
    common = ['--preset', 'vgg300', '--name', str(tmp_path / 'none'), '--threshold', '0.05', '--batch-size', '4']
    assert infer.main(common + ['--output-dir', str(tmp_path / 'plain')] + files) == 0
    plain = [l for l in capsys.readouterr().out.splitlines() if l.startswith('[i] Processed')]
    odir = str(tmp_path / 'drawn')
    assert infer.main(common + ['--annotate', 'true', '--output-dir', odir] + files) == 0
    drawn = [l for l in capsys.readouterr().out.splitlines() if l.startswith('[i] Processed')]
    assert plain == drawn and len(plain) == 1 and plain[0].startswith('[i] Processed 2 images')
    names = ['aeroplane', 'bicycle', 'bird', 'boat', 'bottle', 'bus', 'car', 'cat', 'chair', 'cow', 'diningtable', 'dog', 'horse',
             'motorbike', 'person', 'pottedplant', 'sheep', 'sofa', 'train', 'tvmonitor']
    colors = [ut.default_colors(names)[n] for n in names]
    dets = _detections('vgg300', 20, files, 0.05)
    assert sum(len(d['cls']) for d in dets) > 0
    for f, det in zip(files, dets):
        got = _decode_png(open(os.path.join(odir, os.path.basename(f) + '.png'), 'rb').read())[:, :, ::-1]
        assert got.shape == np.load(f).shape and np.array_equal(got, _expected(f, det, names, colors))


def test_detect_tool(tmp_path, capsys):
    from ssd_tensorflow_amd.ssdvgg import SSDVGG, Session
    model = str(tmp_path / 'model.npz')
    names = ['class_%d' % i for i in range(3)]
    with Session(0) as sess:
        net = SSDVGG(sess, 'vgg300')
        net.build_from_vgg(None, 3, max_batch=2)
        net.build_optimizer()
        net.save_checkpoint(model, class_names=names)
    files = _files(tmp_path, [(300, 300), (240, 352), (100, 90)], seed=9)
    odir = str(tmp_path / 'out')
    assert detect.main(['--model', model, '--output-dir', odir, '--batch-size', '2', '--training-data', 'unused.pkl'] + files) == 0
    dets = _detections('vgg300', 3, files, 0.5, ckpt=model)
    colors = [ut.default_colors(names)[n] for n in names]
    for f, det in zip(files, dets):
        base = os.path.join(odir, os.path.basename(f))
        want = ['{} {} {} {} {} {}\n'.format(b.label, b.labelid, b.center.x, b.center.y, b.size.w, b.size.h)
                for _, b in boxes_from_detection(det, dict(enumerate(names)))]
        assert open(base + '.txt').readlines() == want
        got = _decode_png(open(base + '.png', 'rb').read())[:, :, ::-1]
        assert np.array_equal(got, _expected(f, det, names, colors))


def test_train_writes_image_summaries(tmp_path, capsys):
    run = str(tmp_path / 'run'); tb = str(tmp_path / 'tb')
    assert train.main(['--name', run, '--tensorboard-dir', tb, '--epochs', '2', '--batch-size', '4', '--synthetic-train', '10',
                       '--synthetic-valid', '4', '--checkpoint-interval', '5']) == 0
    for split in ('training', 'validation'):
        d = os.path.join(tb, 'run', split + '_img')
        assert sorted(os.listdir(d)) == ['e2_0.png', 'e2_1.png', 'e2_2.png']
        for f in os.listdir(d):
            assert _decode_png(open(os.path.join(d, f), 'rb').read()).shape == (512, 512, 3)
